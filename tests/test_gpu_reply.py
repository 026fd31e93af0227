"""wsg_reply_messages / wsg_reply_streams on the GPU: frames -> reply frames.

Every call goes through run(): every output starts as a sentinel and d_reply
has SLACK bytes past reply_cap.  Afterwards the reply bytes are checked
against the frames one oracle session per stream sends for its callbacks
(tests/reply_cases.py), the offsets and counts against layout.reply_plan, the
message table, the state and the info against layout.message_plan and
oracle.decode_batch, and everything past the valid entries must still hold
the sentinel.  Damaged wires go through run_damaged(): the same checks
without the sessions, the expected frames built from message_plan over the
oracle's records of the damaged wire."""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests.test_gpu_async import _gate  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402
from tests.test_gpu_messages import PLAN_BLOCK, _three_pass_batch  # noqa: E402

SENTINEL = 0xA5
SLACK = 64   # bytes of d_reply past reply_cap: must stay sentinel whatever happens
EXTRA = 3    # entries of d_reply_off / d_stream_reply past the ones the call may write


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sent(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


class Out:
    """Sentinel-filled outputs of one call over n frames in ns streams."""

    def __init__(self, n, ns, reply_cap, opcodes=None):
        self.n, self.ns, self.cap = n, ns, reply_cap
        st = np.full(max(ns, 1) * STREAM_STATE.itemsize, SENTINEL, dtype=np.uint8).view(STREAM_STATE)
        st["opcode"][:ns] = 0 if opcodes is None else opcodes
        self.state = dev(st.view(np.uint8))
        self.reply = sent(reply_cap + SLACK)
        self.reply_off = sent((n + 1 + EXTRA) * 8).view(torch.int64)
        self.stream_reply = sent((ns + 1 + EXTRA) * 8).view(torch.int64)
        self.msgs = sent(max(n, 1) * MSG.itemsize)
        self.count = sent(4 * 8).view(torch.int64)
        self.info = sent(max(n, 1) * RECV_INFO.itemsize)

    def refill(self, opcodes=None):
        for t in (self.reply, self.reply_off, self.stream_reply, self.msgs, self.count, self.info):
            t.view(torch.uint8).fill_(SENTINEL)
        st = self.state.view(torch.uint8).view(-1, STREAM_STATE.itemsize)
        st[: self.ns, 0:4] = SENTINEL
        st[: self.ns, 4] = 0

    def launch(self, codec, wire, fs, sf, rule, mask, keys, stream=None):
        codec.reply_messages(wire, fs, sf, reply_op=rule, mask=mask, send_keys=keys, state=self.state,
                             reply=self.reply, reply_cap=self.cap, stream=stream, reply_off=self.reply_off,
                             stream_reply=self.stream_reply, msgs=self.msgs, count=self.count, info=self.info)

    def host(self):
        return dict(count=self.count.cpu().numpy(), reply=self.reply.cpu().numpy(),
                    reply_off=self.reply_off.cpu().numpy().view(np.uint64),
                    stream_reply=self.stream_reply.cpu().numpy().view(np.uint64),
                    msgs=self.msgs.cpu().numpy().view(MSG),
                    state=self.state.cpu().numpy().view(STREAM_STATE)[: self.ns],
                    info=self.info.cpu().numpy().view(RECV_INFO)[: self.n])


SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)


def check_outputs(h, n, ns, cap, want_msgs, want_count, want_state, info_o, want_frames, plan, fits=True):
    """One call's outputs on the host against the expected table and frames."""
    reply_off, stream_reply, rcount = plan
    want_bytes = np.frombuffer(b"".join(want_frames), dtype=np.uint8)
    assert [len(f) for f in want_frames] == [int(x) for x in np.diff(reply_off.astype(np.int64))]
    print("count", [int(x) for x in h["count"]], "cap", cap)
    assert [int(x) for x in h["count"]] == [int(want_count[0]), int(want_count[1]), int(rcount[0]), int(rcount[1])]
    nm, need = int(h["count"][0]), int(h["count"][2])
    assert need == len(want_bytes)
    if fits:
        assert need <= cap
        assert np.array_equal(h["reply"][:need], want_bytes)
        assert (h["reply"][need:] == SENTINEL).all()   # the rest of d_reply and the SLACK past reply_cap
    else:
        assert need > cap
        assert (h["reply"] == SENTINEL).all()           # no byte of d_reply is written
    assert np.array_equal(h["reply_off"][: nm + 1], reply_off)
    assert (h["reply_off"][nm + 1:] == SENT64).all()
    assert np.array_equal(h["stream_reply"][: ns + 1], stream_reply)
    assert (h["stream_reply"][ns + 1:] == SENT64).all()
    mc.same_fields(h["info"], info_o, mc.INFO_FIELDS)
    mc.same_fields(h["msgs"][:nm], want_msgs, mc.MSG_FIELDS)
    assert (h["msgs"][nm:].view(np.uint8) == SENTINEL).all() or n == 0
    mc.same_fields(h["state"], want_state, ["consumed", "opcode"])


def expected(batch, rule, mask, keys, state):
    """(message table, counts, state, oracle info, one frame per message, reply_plan)."""
    out_o, info_o = batch.oracle_decode()
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, state, payload=out_o)
    by_stream = rc.oracle_replies(batch, rule, mask, keys, state)
    frames = rc.per_message(want_msgs, by_stream)
    plan = layout.reply_plan(want_msgs, rule, mask, keys, n_streams=batch.n_streams)
    return (want_msgs, want_count, want_state, info_o, frames, plan), by_stream


def d_wire_of(wire):
    return dev(wire) if len(wire) else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]


def d_keys_of(keys):
    return None if keys is None else dev(np.asarray(keys, dtype=np.uint32).view(np.int32))


def run(codec, batch, rule=rc.ECHO, mask=0, keys=None, state=None, reply_cap=None):
    """The call and every check; returns the replies of each stream, as the
    device's d_stream_reply ranges of d_reply."""
    n, ns = batch.n, batch.n_streams
    want, by_stream = expected(batch, rule, mask, keys, state)
    need = int(want[5][2][0])
    assert need <= len(batch.wire) + 14 * n
    cap = len(batch.wire) + 14 * n if reply_cap is None else reply_cap
    o = Out(n, ns, cap, None if state is None else state["opcode"])
    o.launch(codec, d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rule, mask,
             d_keys_of(keys))
    status = codec.sync_status()
    h = o.host()
    check_outputs(h, n, ns, cap, *want, fits=need <= cap)
    if need > cap:
        assert status == ca.WSG_ENOMEM
        assert codec.sync_status() == 0   # reported once
        return None
    assert status == 0
    got = [h["reply"][int(h["stream_reply"][j]): int(h["stream_reply"][j + 1])].tobytes() for j in range(ns)]
    assert got == [b"".join(s) for s in by_stream]
    return got


def run_damaged(codec, batch, wire, fs, rule, mask, keys=None):
    """batch's streams over a damaged `wire`: the expected table from
    message_plan over the oracle's records of that wire, the expected frames
    from that table and the oracle's unmasked bytes."""
    n, ns = batch.n, batch.n_streams
    rc_o, out_o, info_o = oracle.decode_batch(wire, fs)
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, None, payload=out_o)
    buf = mc.dense(out_o, info_o, batch.stream_first, want_state)
    frames = rc.plan_replies(want_msgs, buf, rule, mask, keys)
    plan = layout.reply_plan(want_msgs, rule, mask, keys, n_streams=ns)
    cap = len(wire) + 14 * n
    o = Out(n, ns, cap)
    o.launch(codec, d_wire_of(wire), dev(np.asarray(fs, dtype=np.uint64).view(np.int64)), dev(batch.stream_first),
             rule, mask, d_keys_of(keys))
    status = codec.sync_status()
    check_outputs(o.host(), n, ns, cap, want_msgs, want_count, want_state, info_o, frames, plan)
    assert status == rc_o
    assert codec.sync_status() == 0   # the latch is cleared
    return status


# ------------------------------------------------------- header forms, prefix
@pytest.mark.parametrize("key", [0, rc.KEY4])
@pytest.mark.parametrize("mask", [0, 1])
def test_header_forms_and_prefix(codec, mask, key):
    """Replies with 2/4/10-byte headers (+4 masked), pongs whose two-byte
    prefix moves the body across 125/126 and 65535/65536, at send key 0 and a
    key of four distinct bytes (XORed in when mask == 0 too)."""
    batch = mc.Batch([rc.header_form_stream(np.random.default_rng(10))])
    (got,) = run(codec, batch, rc.ECHO, mask, [key])
    if not mask and not key:   # Q2 on the first non-empty ping: 8A, length 3, 00 00, the byte
        pongs = got[sum(len(f) for f in rc.oracle_replies(batch, rc.ECHO, 0, [0])[0][:8]):]
        assert pongs[:4] == b"\x8a\x03\x00\x00"
    run(codec, batch, rc.EVERYTHING, mask, [key])   # pings with a prefix in reply to data


def test_q2_literal(codec):
    batch = mc.Batch([[mc.raw_frame(0x89, b"ab", key=0x11223344)]])
    assert run(codec, batch) == [bytes.fromhex("8A0400006162")]


# ------------------------------------------------------ alignment, key phase
def _align_frames(rng):
    frames = [mc.raw_frame(0x82, rc.data(rng, n), key=int(rng.integers(1, 2**32)) if i & 1 else None)
              for i, n in enumerate((1, 15, 16, 17, 31, 127, 4097))]
    frames += rc.fragments(rng, 0x82, [1, 2, 3, 5, 4097])
    frames += rc.fragments(rng, 0x89, [1, 2, 3, 5, 4097])   # the prefix shifts the send phase by 2
    frames += rc.fragments(rng, 0x81, [5, 4097, 3, 2, 1])
    return frames


@pytest.mark.parametrize("front", [0, 1, 2, 3])
def test_alignment_and_key_phase(codec, front):
    """tests/test_gpu_messages.py::test_edge_shapes' scheme, a frame of `front`
    bytes ahead, shifts every source; the next reply, of 2..17 bytes, puts the
    rest at every destination alignment mod 16; fragments of 1, 2, 3, 5 and
    4097 bytes, each with its own receive key, walk the combined key's phase,
    in a ping too."""
    rng = np.random.default_rng(20 + front)
    body = _align_frames(rng)
    ahead = [mc.raw_frame(0x81, bytes(range(front)), key=0x01020304)] if front else []
    starts = set()
    for lead in range(2, 18):
        first = mc.raw_frame(0x82, rc.data(rng, lead - 2), key=int(rng.integers(1, 2**32)))
        batch = mc.Batch([[mc.raw_frame(0x01, b"t")], ahead + [first] + body])   # (a tail-only stream: odd source shifts)
        got = run(codec, batch, rc.SAME_CLOSE_PONG, lead & 1, [7, rc.KEY4])
        at = (2 + front + (4 if lead & 1 else 0) if front else 0) + lead + (4 if lead & 1 else 0)
        assert got[0] == b"" and len(got[1]) > 3 * 4097 and got[1][at] == 0x82   # the reply behind the lead's
        starts.add(at % 16)
    assert len(starts) == 16


# --------------------------------------------------------------------- pieces
@pytest.mark.parametrize("size", [4095, 4096, 4097, 3 * 4096 + 1])
def test_piece_boundaries(codec, size):
    rng = np.random.default_rng(size)
    whole = [mc.raw_frame(0x82, rc.data(rng, size), key=int(rng.integers(1, 2**32)))]
    for cut in (1, size // 2, 4096 if size > 4096 else size - 1):
        two = rc.fragments(rng, 0x82, [cut, size - cut])
        ping = rc.fragments(rng, 0x89, [size - cut, cut])
        for mask in (0, 1):
            run(codec, mc.Batch([whole + two, ping + whole]), rc.ECHO, mask, [rc.KEY4, 0x01020304])


# --------------------------------------------------------------------- quirks
def _quirk_batch():
    q = mc.quirk_streams()
    names = sorted(q)
    streams = [q[k] for k in names] + [[mc.raw_frame(0x88, b"\x00\x00why", key=3)]]   # a close whose status is 0
    return mc.Batch(streams), names


@pytest.mark.parametrize("rule", ["echo", "same_close_pong", "none"])
@pytest.mark.parametrize("mask", [0, 1])
def test_quirks(codec, rule, mask):
    batch, names = _quirk_batch()
    keys = np.arange(batch.n_streams, dtype=np.uint32) * 0x01010101 + rc.KEY4
    got = run(codec, batch, rc.RULES[rule], mask, keys)
    if rule == "none":
        assert got == [b""] * batch.n_streams
    if rule == "same_close_pong" and not mask:
        k = lambda j: np.frombuffer(int(keys[j]).to_bytes(4, "little"), np.uint8)  # noqa: E731
        j = names.index("close_status_split")
        assert got[j] == b"\x88\x02" + (np.frombuffer(b"\x03\xe9", np.uint8) ^ k(j)[:2]).tobytes()
        j = names.index("close_one_byte")
        assert got[j] == b"\x88\x02" + (np.frombuffer(b"\x03\xe8", np.uint8) ^ k(j)[:2]).tobytes()
        assert got[names.index("close_empty")][:2] == b"\x88\x02"
        assert got[-1] == b"\x88\x00"   # status 0: PrepareSendFrame(op, mask, NULL, 0, 0) has no prefix


# -------------------------------------------------------------------- streams
def test_streams_without_replies(codec):
    rng = np.random.default_rng(30)
    pongs = [mc.raw_frame(0x8A, rc.data(rng, n), key=9 + n) for n in (0, 5, 130)]
    tail = [mc.raw_frame(0x02, b"open", key=1), mc.raw_frame(0x00, b"...")]
    msg = [mc.raw_frame(0x81, b"hello", key=77)]
    batch = mc.Batch([[], msg, [], tail, pongs, msg + tail, [], msg, []])
    got = run(codec, batch, rc.ECHO, 0, None)
    assert [len(g) for g in got] == [0, 7, 0, 0, 0, 7, 0, 7, 0]
    run(codec, batch, rc.EVERYTHING, 1, np.arange(9) + 1)
    run(codec, mc.Batch([[], tail, pongs]))    # frames, no reply at all
    run(codec, mc.Batch([]))                   # n == 0, n_streams == 0
    run(codec, mc.Batch([[], [], []]))         # n == 0
    st = np.zeros(2, dtype=STREAM_STATE)       # a seeded ping continues: the pong carries all of it
    st["opcode"] = [9, 2]
    got = run(codec, mc.Batch([[mc.raw_frame(0x80, b"rest", key=4)], [mc.raw_frame(0x00, b"tail")]]), state=st)
    assert got == [b"\x8a\x06\x00\x00rest", b""]


@pytest.mark.parametrize("seed", range(4))
def test_carry_over(codec, seed):
    """Each stream's frame list cut at a random frame into two calls, the
    second taking the first's tail, the rest and the returned opcode: the two
    calls' replies together are the one call's."""
    rng = np.random.default_rng(40 + seed)
    streams = [mc.random_frames(rng, int(rng.integers(0, 14)), 3000) for _ in range(int(rng.integers(2, 9)))]
    keys = rng.integers(0, 2**32, len(streams)).astype(np.uint32)
    rule, mask = rc.SAME_CLOSE_PONG, seed & 1
    whole = run(codec, mc.Batch(streams), rule, mask, keys)
    cuts = [int(rng.integers(0, len(s) + 1)) for s in streams]
    first = mc.Batch([s[:c] for s, c in zip(streams, cuts)])
    r1 = run(codec, first, rule, mask, keys)
    _, info = first.oracle_decode()
    _, _, st1 = layout.message_plan(info, first.stream_first, None)   # (run checked the device's against it)
    rest = [s[int(st1["consumed"][j]):] for j, s in enumerate(streams)]
    r2 = run(codec, mc.Batch(rest), rule, mask, keys, state=st1.copy())
    assert [a + b for a, b in zip(r1, r2)] == whole


# ---------------------------------------------------- scans past one block
def _tiny_streams(rng, n, ns):
    frames = []
    for i in range(n):
        op = int(rng.choice([0, 1, 2, 9, 10, 8, 3]))
        fin = 0x80 if rng.random() < 0.6 else 0
        frames.append(mc.raw_frame(fin | op, rc.data(rng, int(rng.integers(1, 9))),
                                   key=int(rng.integers(0, 2**32)) if rng.random() < 0.7 else None))
    cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, ns - 1)), [n]])
    return [frames[cuts[j]: cuts[j + 1]] for j in range(ns)]


def test_scans_past_one_block_and_grid_stride():
    """3 * 256 + 5 tiny frames in 7 streams: the reply scans cross block
    boundaries and use the block partials.  In a context with one block per
    CU the gather has 4 waves per CU; a second batch of the same kind sized
    from the CU count has more pieces than that, so the grid-stride loop's
    second pass runs over reply pieces."""
    c = _codec(WSG_ENC_BLOCKS_PER_CU=1)
    try:
        rng = np.random.default_rng(50)
        batch = mc.Batch(_tiny_streams(rng, 3 * 256 + 5, 7))
        assert batch.n == 3 * 256 + 5 and batch.n_streams == 7
        keys = rng.integers(0, 2**32, 7).astype(np.uint32)
        run(c, batch, rc.SAME_CLOSE_PONG, 1, keys)
        run(c, batch, rc.ECHO, 0, None)
        waves = 4 * int(torch.cuda.get_device_properties(0).multi_processor_count)
        big = mc.Batch(_tiny_streams(rng, 2 * waves + 5, 7))
        _, info = big.oracle_decode()
        _, _, st = layout.message_plan(info, big.stream_first, None)
        delivered = np.zeros(big.n, dtype=bool)
        for j in range(7):
            lo = int(big.stream_first[j])
            delivered[lo: lo + int(st["consumed"][j])] = True
        pieces = int((delivered & (info["len"] > 0)).sum())   # one piece or two per such frame
        assert pieces > waves
        run(c, big, rc.SAME_CLOSE_PONG, 0, keys)
    finally:
        c.close()


def test_reply_scans_three_passes(codec):
    """tests/test_gpu_messages.py's three-pass batch (131 716 frames: three
    passes of 256 block partials) as replies.  Messages end in passes one and
    three of the partials and none in pass two, so k_reply_blocks' two
    carries, reply bytes and reply frames, come through a pass that adds
    nothing to either, and the prefixes of pass three hold pass one's sum."""
    batch, _ = _three_pass_batch()
    rule, mask = rc.SAME_CLOSE_PONG, 1
    keys = np.random.default_rng(55).integers(0, 2**32, batch.n_streams).astype(np.uint32)
    out_o, info_o = batch.oracle_decode()
    msgs, _, _ = layout.message_plan(info_o, batch.stream_first, None, payload=out_o)
    reply_off, _, rcount = layout.reply_plan(msgs, rule, mask, keys, n_streams=batch.n_streams)
    per_pass = PLAN_BLOCK * PLAN_BLOCK   # frames whose block partials one pass scans
    assert 2 * per_pass < batch.n <= 3 * per_pass
    ends = msgs["first_frame"].astype(np.int64) + msgs["nframes"] - 1   # the FIN frame: where the reply is counted
    size = np.diff(reply_off.astype(np.int64))
    in_pass = [(ends >= k * per_pass) & (ends < (k + 1) * per_pass) for k in range(3)]
    for k in range(3):
        print("pass", k + 1, "messages", int(in_pass[k].sum()), "reply frames", int((size[in_pass[k]] > 0).sum()),
              "reply bytes", int(size[in_pass[k]].sum()))
    assert not in_pass[1].any()
    assert (size[in_pass[0]] > 0).any() and (size[in_pass[2]] > 0).any()
    assert int(size.sum()) == int(rcount[0]) and int((size > 0).sum()) == int(rcount[1])
    run(codec, batch, rule, mask, keys)


# ------------------------------------------------------------------ capacity
def test_reply_cap_one_byte_short(codec):
    rng = np.random.default_rng(60)
    frames = [mc.raw_frame(0x82, rc.data(rng, 700 + i), key=5 + i) for i in range(9)]
    batch = mc.Batch([frames[:4] + [mc.raw_frame(0x89, b"pp", key=1)], frames[4:] + [mc.raw_frame(0x02, b"tail")]])
    need = sum(4 + 700 + i for i in range(9)) + 6
    assert run(codec, batch, reply_cap=need - 1) is None    # WSG_ENOMEM, once; d_reply untouched; the counts hold the need
    got = run(codec, batch, reply_cap=need)
    assert sum(len(g) for g in got) == need


# -------------------------------------------------------------------- damage
@pytest.mark.parametrize("seed", range(6))
def test_damaged_wires(codec, seed):
    """tests/test_gpu_messages.py::test_fuzz's damage: one to three wire
    bytes overwritten, the wire cut short with probability 0.3, the same frame
    table; and the wire cut inside its last frame."""
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
    run_damaged(codec, batch, bad, batch.fs, rule, seed & 1, keys)
    cut = batch.wire[: len(batch.wire) - 1 - int(rng.integers(0, len(streams[-1][-1]) - 1))]
    assert run_damaged(codec, batch, cut, batch.fs, rule, seed & 1, keys) == ca.WSG_ETRUNC


# --------------------------------------------------------------------- async
def _two_batches():
    """The same frames in another order over other stream boundaries:
    wire_len, n and n_streams agree, the geometry does not."""
    rng = np.random.default_rng(80)
    n, ns = 600, 6
    frames = mc.random_frames(rng, n, 1500)
    out = []
    for k in range(2):
        order = np.arange(n) if k == 0 else rng.permutation(n)
        cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, ns - 1)), [n]])
        fr = [frames[i] for i in order]
        out.append(mc.Batch([fr[cuts[j]: cuts[j + 1]] for j in range(ns)]))
    assert len(out[0].wire) == len(out[1].wire) and int((out[0].fs != out[1].fs).sum()) > n // 2
    return out


def test_two_streams_one_context():
    """(batch A on S1, batch B on S2) four times on one context, all queued
    while a sleeping kernel holds both streams back: the calls share the plan
    block and the piece records, and the library orders them on the device."""
    codec = ca.Codec(0)
    try:
        batches = _two_batches()
        keys = np.arange(6, dtype=np.uint32) * 0x11111111 + 5
        rule, mask = rc.SAME_CLOSE_PONG, 1
        wants = [expected(b, rule, mask, keys, None)[0] for b in batches]
        n, ns, cap = batches[0].n, 6, len(batches[0].wire) + 14 * batches[0].n
        ins = [(dev(b.wire), dev(b.fs.view(np.int64)), dev(b.stream_first)) for b in batches]
        d_keys = d_keys_of(keys)
        for i, w in zip(ins, wants):   # sized, and each batch checked on its own
            o = Out(n, ns, cap)
            o.launch(codec, *i, rule, mask, d_keys)
            assert codec.sync_status() == 0
            check_outputs(o.host(), n, ns, cap, *w)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [(Out(n, ns, cap), Out(n, ns, cap)) for _ in range(4)]
        torch.cuda.synchronize()
        gate = _gate([s1, s2])
        for oa, ob in outs:
            oa.launch(codec, *ins[0], rule, mask, d_keys, s1)
            ob.launch(codec, *ins[1], rule, mask, d_keys, s2)
        opened = gate.query()
        assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
        torch.cuda.synchronize()
        assert not opened, "the gate opened before every call was queued"
        for pair in outs:
            for o, w in zip(pair, wants):
                check_outputs(o.host(), n, ns, cap, *w)
    finally:
        codec.close()


def test_graph_replay():
    """One call captured after a warm run with the same n, replayed twice on
    new payload bytes and receive keys of the same geometry."""
    codec = ca.Codec(0)
    try:
        fixed = np.random.default_rng(90)
        lens = fixed.choice([0, 1, 5, 300, 5000], 120)
        b0s = fixed.choice([0x82, 0x81, 0x89, 0x02, 0x00, 0x80, 0x8A], 120)
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
            check_outputs(o.host(), n, ns, cap, *expected(b, rule, mask, keys, None)[0])
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
                check_outputs(o.host(), n, ns, cap, *expected(b, rule, mask, keys, None)[0])
    finally:
        codec.close()


# -------------------------------------------------------------- reply_streams
def test_reply_streams(codec):
    """Raw spans with partial tails to reply frames: the replies of each
    connection against one oracle session fed its whole frames, consumed
    lowered to the first tail frame as wsg_decode_streams does, WSG_EINVAL
    while capturing."""
    rng = np.random.default_rng(100)
    lists = [mc.random_frames(rng, int(rng.integers(0, 9)), 500) for _ in range(12)]
    lists[3] = [mc.raw_frame(0x89, b"ab", key=1), mc.raw_frame(0x02, b"open", key=2), mc.raw_frame(0x00, b"more")]
    partial = [mc.raw_frame(0x82, rc.data(rng, 200), key=3)[: int(c)] for c in rng.integers(0, 150, 12)]
    w = fc.Wire([b"".join(f) + p for f, p in zip(lists, partial)])
    ns, cap = 12, len(w.wire) // 2
    keys = rng.integers(0, 2**32, ns).astype(np.uint32)
    keys[3] = 0
    rule, mask = rc.SAME_CLOSE_PONG, 0
    d_wire, d_keys = dev(w.wire), d_keys_of(keys)
    batch = mc.Batch(lists)    # the whole frames, for the expected replies
    by_stream = rc.oracle_replies(batch, rule, mask, keys)
    plan = layout.frame_plan(w.wire, w.spans)
    assert int(plan[3][0]) == batch.n

    def outputs():
        o = Out(cap, ns, len(w.wire) + 14 * cap)
        o.spans = dev(w.spans.view(np.uint8))
        o.fs = sent(cap * 8).view(torch.int64)
        o.sf = sent((ns + 1) * 4).view(torch.int32)
        return o

    def call(o, stream=None):
        return codec.reply_streams(d_wire, o.spans, reply_op=rule, mask=mask, send_keys=d_keys,
                                   state=o.state, frame_start=o.fs, frame_cap=cap, stream_first=o.sf, reply=o.reply,
                                   reply_cap=o.cap, stream=stream, reply_off=o.reply_off,
                                   stream_reply=o.stream_reply, msgs=o.msgs, count=o.count, info=o.info)[-1]

    o = outputs()
    assert call(o) == batch.n
    assert codec.sync_status() == 0
    o.n = batch.n
    h = o.host()
    out_o, info_o = batch.oracle_decode()
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, None, payload=out_o)
    rplan = layout.reply_plan(want_msgs, rule, mask, keys, n_streams=ns)
    assert [int(x) for x in h["count"]] == [int(want_count[0]), int(want_count[1]), int(rplan[2][0]), int(rplan[2][1])]
    got = [h["reply"][int(h["stream_reply"][j]): int(h["stream_reply"][j + 1])].tobytes() for j in range(ns)]
    assert got == [b"".join(s) for s in by_stream]
    assert got[3] == b"\x8a\x04\x00\x00ab"
    assert (h["reply"][int(h["count"][2]):] == SENTINEL).all()
    assert np.array_equal(h["reply_off"][: int(h["count"][0]) + 1], rplan[0])
    mc.same_fields(h["state"], want_state, ["consumed", "opcode"])
    spans = o.spans.cpu().numpy().view(STREAM_SPAN)
    assert np.array_equal(spans["need"], plan[2]["need"])
    lowered_any = False
    for j in range(ns):
        first, used = int(plan[1][j]), int(want_state["consumed"][j])
        nj = int(plan[1][j + 1]) - first
        lowered = int(plan[0][first + used]) - int(w.spans["off"][j]) if used < nj else int(plan[2]["consumed"][j])
        lowered_any |= used < nj
        assert int(spans["consumed"][j]) == lowered, "stream %d" % j
    assert lowered_any
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        o = outputs()
        assert call(o) == batch.n   # sized, outside the capture
        assert codec.sync_status() == 0
        with torch.cuda.graph(g, stream=st):
            o.count.fill_(-1)       # (a node, so that the capture is not empty)
            with pytest.raises(ca.WSGError) as e:
                call(o)
        assert e.value.code == ca.WSG_EINVAL
