"""wsg_decode_messages on the GPU: frames -> messages, packed densely.

Every call goes through run(): d_msg, d_msgs and d_state start as a sentinel;
afterwards the message bytes and the table are checked against one oracle
session per stream (kind, data, status of every callback, in order), the table
and the state against layout.message_plan, info against oracle.decode_batch,
and every byte of d_msg at or after count[1] (and every record at or after
count[0]) must still hold the sentinel.  Damaged wires go through
run_damaged(): the same checks without the sessions, the expected values taken
from the oracle's records of the damaged wire."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout, workloads as wl  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_STATE  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402
from tests.test_gpu_parity import _frames_wire  # noqa: E402

SENTINEL = 0xA5
SLACK = 64   # bytes of d_msg past msg_cap: must stay sentinel whatever happens


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(codec, batch, state=None):
    """The call and every check; returns (msgs, msg bytes, new state)."""
    n, ns = batch.n, batch.n_streams
    cap = len(batch.wire)
    st = np.full(max(ns, 1) * STREAM_STATE.itemsize, SENTINEL, dtype=np.uint8).view(STREAM_STATE)
    st["opcode"][:ns] = 0 if state is None else state["opcode"]
    d_state = dev(st.view(np.uint8))
    d_msg = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msgs = torch.full((max(n, 1) * MSG.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    d_info = torch.full((max(n, 1) * RECV_INFO.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    wire = dev(batch.wire) if len(batch.wire) else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    codec.decode_messages(wire, dev(batch.fs.view(np.int64)), dev(batch.stream_first), state=d_state, msg=d_msg,
                          msg_cap=cap, msgs=d_msgs, count=d_count, info=d_info)
    assert codec.sync_status() == 0
    count = d_count.cpu().numpy()
    msg = d_msg.cpu().numpy()
    msgs_all = d_msgs.cpu().numpy().view(MSG)
    new_state = d_state.cpu().numpy().view(STREAM_STATE)[:ns]
    info = d_info.cpu().numpy().view(RECV_INFO)[:n]

    out_o, info_o = batch.oracle_decode()
    mc.same_fields(info, info_o, mc.INFO_FIELDS)
    in_state = None if state is None else state
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, in_state, payload=out_o)
    assert [int(x) for x in count] == [int(x) for x in want_count]
    msgs = msgs_all[: int(count[0])]
    mc.same_fields(msgs, want_msgs, mc.MSG_FIELDS)
    assert (msgs_all[int(count[0]):].view(np.uint8) == SENTINEL).all() or n == 0
    mc.same_fields(new_state, want_state, ["consumed", "opcode"])
    used = int(count[1])
    assert np.array_equal(msg[:used], mc.dense(out_o, info_o, batch.stream_first, want_state))
    assert (msg[used:] == SENTINEL).all()
    mc.check_events(batch, msgs, msg[:used], new_state, info_o, in_state)
    return msgs, msg[:used], new_state


def _call_sentinel(codec, batch, wire, fs, msg_cap):
    """One call on sentinel-filled outputs; returns (status, count, msg with
    its SLACK, every MSG record, state, info) on the host."""
    n, ns = batch.n, batch.n_streams
    d_state = torch.zeros(max(ns, 1) * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    d_msg = torch.full((msg_cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msgs = torch.full((max(n, 1) * MSG.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    d_info = torch.full((max(n, 1) * RECV_INFO.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_wire = dev(wire) if len(wire) else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    codec.decode_messages(d_wire, dev(np.asarray(fs, dtype=np.uint64).view(np.int64)), dev(batch.stream_first),
                          state=d_state, msg=d_msg, msg_cap=msg_cap, msgs=d_msgs, count=d_count, info=d_info)
    status = codec.sync_status()
    return (status, d_count.cpu().numpy(), d_msg.cpu().numpy(), d_msgs.cpu().numpy().view(MSG),
            d_state.cpu().numpy().view(STREAM_STATE)[:ns], d_info.cpu().numpy().view(RECV_INFO)[:n])


def run_damaged(codec, batch, wire, fs):
    """batch's streams over a damaged `wire` (bytes overwritten, cut short) with
    the frame table `fs`, msg_cap = len(wire).  A frame error is latched and
    the frame counts as an empty non-FIN continuation (wsg_capi.h), which is
    what layout.message_plan makes of the oracle's record of such a frame:
    info and status against oracle.decode_batch, table, counts and state
    against message_plan over that info, bytes against mc.dense, and the
    sentinel everywhere past them.  No per-stream session is consulted: a
    session misreads a damaged stream in its own way."""
    cap = len(wire)
    status, count, msg, msgs_all, new_state, info = _call_sentinel(codec, batch, wire, fs, cap)
    rc_o, out_o, info_o = oracle.decode_batch(wire, fs)
    mc.same_fields(info, info_o, mc.INFO_FIELDS)
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, None, payload=out_o)
    assert [int(x) for x in count] == [int(x) for x in want_count]
    used = int(count[1])
    assert used <= cap   # valid frames of a sorted table hold disjoint ranges of the wire
    assert status == rc_o
    mc.same_fields(msgs_all[: int(count[0])], want_msgs, mc.MSG_FIELDS)
    assert (msgs_all[int(count[0]):].view(np.uint8) == SENTINEL).all() or batch.n == 0
    mc.same_fields(new_state, want_state, ["consumed", "opcode"])
    assert np.array_equal(msg[:used], mc.dense(out_o, info_o, batch.stream_first, want_state))
    assert (msg[used:] == SENTINEL).all()   # the rest of d_msg and the SLACK past msg_cap
    assert codec.sync_status() == 0         # the latch is cleared
    return status, info_o


EDGE_LENGTHS = [0, 1, 15, 16, 17, 125, 126, 127, 4095, 4096, 4097, 65535, 65536]


def _edge_frames(rng):
    frames = []
    for n in EDGE_LENGTHS:
        for masked in (True, False):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            frames.append(mc.raw_frame(0x82, data, key=int(rng.integers(1, 2**32)) if masked else None))
    return frames


@pytest.mark.parametrize("front", [0, 1, 2, 3])
def test_edge_shapes(codec, front):
    """Single-frame messages of the edge lengths, masked and unmasked (2/4/6/
    8/10/14-byte headers), behind a frame of `front` bytes: the source and
    destination alignments and the key phase."""
    rng = np.random.default_rng(100 + front)
    frames = _edge_frames(rng)
    if front:
        frames = [mc.raw_frame(0x81, bytes(range(front)), key=0x01020304)] + frames
    msgs, _, _ = run(codec, mc.Batch([frames]))
    assert len(msgs) == len(frames) and (msgs["nframes"] == 1).all()


def test_edge_shapes_key_zero_and_shuffled(codec):
    """Masked frames with key 0 are plain copies; the edge lengths in another order."""
    rng = np.random.default_rng(104)
    frames = [mc.raw_frame(0x82, rng.integers(0, 256, n, dtype=np.uint8).tobytes(), key=0) for n in EDGE_LENGTHS]
    more = _edge_frames(rng)
    rng.shuffle(more)
    run(codec, mc.Batch([frames, more]))


@pytest.mark.parametrize("a", range(16))
def test_alignment_sweep(codec, a):
    """An unmasked filler frame of a bytes, then a message of a b-byte fragment
    and a 5000-byte fragment (it crosses a piece boundary and shares both edge
    chunks with its neighbours), for b in 0..15.  Header sizes are even, so a
    tail-only stream in front of odd size walks the odd source shifts too."""
    rng = np.random.default_rng(200 + a)
    for b in range(16):
        t = (3 * a + 7 * b) % 16
        tail = [mc.raw_frame(0x01, bytes(t))]
        filler = mc.raw_frame(0x82, rng.integers(0, 256, a, dtype=np.uint8).tobytes())
        f1 = mc.raw_frame(0x02, rng.integers(0, 256, b, dtype=np.uint8).tobytes(),
                          key=int(rng.integers(1, 2**32)) if (a + b) & 1 else None)
        f2 = mc.raw_frame(0x80, rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), key=int(rng.integers(1, 2**32)))
        after = mc.raw_frame(0x82, b"next", key=77)
        msgs, buf, state = run(codec, mc.Batch([tail, [filler, f1, f2, after]]))
        assert list(msgs["len"]) == [a, b + 5000, 4] and list(state["consumed"]) == [0, 4]


def test_fragment_and_quirk_cases(codec):
    q = mc.quirk_streams()
    for name in sorted(q):
        run(codec, mc.Batch([q[name]]))
    streams = [[]]
    for name in sorted(q):
        streams += [q[name], []]
    msgs, buf, state = run(codec, mc.Batch(streams))
    ev = mc.events_by_stream(msgs, buf, len(streams))
    names = sorted(q)
    assert ev[1 + 2 * names.index("continuation_after_fin")] == [(1, b"hello world", 0), (1, b"again", 0)]
    assert ev[1 + 2 * names.index("close_status_split")] == [(2, b"gone", 1001)]
    assert ev[1 + 2 * names.index("close_one_byte")] == [(2, b"\x03", 1000)]
    assert ev[1 + 2 * names.index("rfc_fragmented_hello")] == mc.kat_stream("rfc_fragmented_hello")[1]
    assert ev[1 + 2 * names.index("q5_continuation_concat")] == mc.kat_stream("q5_continuation_concat")[1]


def test_no_frames_and_no_streams(codec):
    run(codec, mc.Batch([]))
    run(codec, mc.Batch([[], [], []]))
    # a seeded opcode comes back unchanged when nothing is consumed
    st = np.zeros(2, dtype=STREAM_STATE)
    st["opcode"] = [9, 2]
    _, _, new = run(codec, mc.Batch([[], [mc.raw_frame(0x00, b"tail")]]), st)
    assert list(new["opcode"]) == [9, 2] and list(new["consumed"]) == [0, 0]


def test_many_streams(codec):
    """1000 streams of 0-3 tiny frames, about a third ending in a tail."""
    rng = np.random.default_rng(300)
    streams = []
    for _ in range(1000):
        k = int(rng.integers(0, 4))
        frames = []
        for i in range(k):
            last = i == k - 1
            fin = 0x80 if (not last or rng.random() > 1 / 3) else 0x00
            op = int(rng.choice([0, 1, 2, 8, 9, 10, 3]))
            data = rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes()
            frames.append(mc.raw_frame(fin | op, data, key=int(rng.integers(0, 2**32)) if rng.random() < 0.7 else None))
        streams.append(frames)
    msgs, _, state = run(codec, mc.Batch(streams))
    tails = sum(int(state["consumed"][j]) < len(s) for j, s in enumerate(streams))
    assert 150 < tails < 450 and len(msgs) > 800


def test_one_stream_of_4096_frames(codec):
    """Every frame in one stream: the scans cross block boundaries inside a
    stream, with runs of continuations longer than a block."""
    rng = np.random.default_rng(301)
    frames = []
    for i in range(4096):
        fin = 0x80 if (rng.random() < 0.3 and not 1000 <= i < 1700) else 0x00
        op = int(rng.choice([0, 0, 0, 1, 2, 9, 8])) if not 2000 <= i < 2600 else 0
        data = rng.integers(0, 256, int(rng.integers(0, 64)), dtype=np.uint8).tobytes()
        frames.append(mc.raw_frame(fin | op, data, key=int(rng.integers(0, 2**32)) if rng.random() < 0.7 else None))
    msgs, _, _ = run(codec, mc.Batch([frames]))
    assert int(msgs["nframes"].max()) > 700


PLAN_BLOCK = 256          # wsg_internal.h: frames per block of the plan's local scans
LONG_FIRST = 60000        # the long stream's first frame
LONG_CONTINUATIONS = 71700


@functools.lru_cache(maxsize=None)
def _three_pass_batch():
    """n = 2 * 65 536 + ~700 frames of 0-8 payload bytes: the plan's scans of
    the per-block partials (k_msg_scan_blocks, k_msg_bytes_blocks: 256
    partials a pass) run three passes, and each carry has to come through a
    pass that adds nothing to it.
      frames [0, 60 000): streams of 1-3 frames, opcodes mixed, about a third
        ending in a tail frame;
      one long stream: frame 59 999 is a whole text message (so the long
        message's first frame comes from the last-FIN-before carry, not from
        the stream's start), frame 60 000 is 0x02 non-FIN, 71 700 frames 0x00
        non-FIN follow (every frame of pass two, 65 536..131 071, is one of
        them: no FIN and no named opcode there), a 0x80 FIN, and two more 0x80
        messages whose opcode is still 2;
      then a few small streams and a tail-only stream.
    The frames are built here (raw_frame's layout for payloads under 126
    bytes) from bulk random draws: raw_frame per frame took 3 s."""
    rng = np.random.default_rng(700)
    total = LONG_FIRST + LONG_CONTINUATIONS + 64
    lens = rng.integers(0, 9, total)
    keys = rng.integers(0, 2**32, total)
    masked = rng.random(total) < 0.7
    pool = rng.integers(0, 256, 8 * total, dtype=np.uint8).tobytes()
    ops = rng.choice([0, 1, 2, 8, 9, 10, 3], total)
    at = [0]

    def frame(b0):
        i = at[0]
        at[0] += 1
        data = pool[8 * i: 8 * i + int(lens[i])]
        if not masked[i]:
            return bytes([b0, len(data)]) + data
        kb = int(keys[i]).to_bytes(4, "little")
        return bytes([b0, 0x80 | len(data)]) + kb + bytes(a ^ b for a, b in zip(data, kb + kb))

    def small_stream(k):
        tail = rng.random() < 1 / 3
        return [frame((0x00 if tail and i == k - 1 else 0x80) | int(ops[at[0]])) for i in range(k)]

    streams = []
    while at[0] < LONG_FIRST - 1:
        streams.append(small_stream(min(int(rng.integers(1, 4)), LONG_FIRST - 1 - at[0])))
    long_stream = len(streams)
    streams.append([frame(0x81), frame(0x02)] + [frame(0x00) for _ in range(LONG_CONTINUATIONS)] +
                   [frame(0x80), frame(0x80), frame(0x80)])
    streams += [small_stream(int(rng.integers(1, 4))) for _ in range(6)]
    streams.append([frame(0x01)])   # a tail-only stream
    assert at[0] <= total
    return mc.Batch(streams), long_stream


def _check_three_pass_batch(batch, long_stream):
    """The batch reaches the passes it is for."""
    n = batch.n
    assert n > 2 * PLAN_BLOCK * PLAN_BLOCK      # three passes over the block partials
    assert int(batch.stream_first[long_stream]) == LONG_FIRST - 1
    _, info = batch.oracle_decode()
    two = slice(PLAN_BLOCK * PLAN_BLOCK, 2 * PLAN_BLOCK * PLAN_BLOCK)
    assert not info["fin"][two].any() and not info["opcode"][two].any()   # pass two adds nothing to cq, cp
    assert info["fin"][: two.start].any() and info["fin"][two.stop:].any()


def _check_long_message(msgs, long_stream):
    long_msgs = msgs[msgs["stream"] == long_stream]
    assert list(long_msgs["opcode"]) == [1, 2, 2, 2] and (long_msgs["kind"] == ca.CB_RECEIVED).all()
    assert int(long_msgs["first_frame"][1]) == LONG_FIRST and int(long_msgs["nframes"][1]) > 71000
    assert list(long_msgs["nframes"][[0, 2, 3]]) == [1, 1, 1]


def test_plan_scans_three_passes(codec):
    """The carries of the plan's block scans over three passes: the last FIN
    before (cq) and the sticky opcode (cp) from pass one through a pass two
    that holds no FIN frame and no named opcode into pass three; the FIN count
    (cf), byte offsets (cb) and piece counts across both pass boundaries.
    Every stream is checked against its own oracle session (0.6 s)."""
    batch, long_stream = _three_pass_batch()
    _check_three_pass_batch(batch, long_stream)
    msgs, _, state = run(codec, batch)
    _check_long_message(msgs, long_stream)
    assert int(state["consumed"][long_stream]) == LONG_CONTINUATIONS + 5 and int(state["opcode"][long_stream]) == 2


def test_gather_grid_stride():
    """k_msg_gather's loop over pieces: a context with one block per CU
    ($WSG_ENC_BLOCKS_PER_CU=1: 4 waves per CU) takes the three-pass batch's
    pieces, one or more per non-empty delivered frame, many per wave; then
    the edge lengths and a 70 001-byte frame, whose 17-18 piece records the
    whole wave writes."""
    batch, long_stream = _three_pass_batch()
    c = _codec(WSG_ENC_BLOCKS_PER_CU=1)
    try:
        waves = 4 * int(torch.cuda.get_device_properties(0).multi_processor_count)
        _, info = batch.oracle_decode()
        _, _, want_state = layout.message_plan(info, batch.stream_first, None)
        delivered = np.zeros(batch.n, dtype=bool)
        for j in range(batch.n_streams):
            lo = int(batch.stream_first[j])
            delivered[lo: lo + int(want_state["consumed"][j])] = True
        pieces = int((delivered & (info["len"] > 0)).sum())   # at least: one piece or two per such frame
        assert pieces > 3 * waves
        msgs, _, _ = run(c, batch)
        _check_long_message(msgs, long_stream)
        rng = np.random.default_rng(701)
        frames = _edge_frames(rng) + [mc.raw_frame(0x82, rng.integers(0, 256, 70001, dtype=np.uint8).tobytes(),
                                                   key=0xA1B2C3D4)]
        rng.shuffle(frames)
        small = mc.Batch([frames[:9], frames[9:]])
        run(c, small)
    finally:
        c.close()


@pytest.mark.parametrize("seed", range(8))
def test_carry_over(codec, seed):
    """Each stream's frame list cut at a random point into two calls; the second
    takes the first's tail (by consumed), the rest and the returned state.  The
    two calls' messages together are what one oracle session delivers."""
    rng = np.random.default_rng(400 + seed)
    streams = [mc.random_frames(rng, int(rng.integers(0, 14)), 3000) for _ in range(int(rng.integers(1, 10)))]
    cuts = [int(rng.integers(0, len(s) + 1)) for s in streams]
    m1, b1, st1 = run(codec, mc.Batch([s[:c] for s, c in zip(streams, cuts)]))
    rest = [s[int(st1["consumed"][j]):] for j, s in enumerate(streams)]
    m2, b2, st2 = run(codec, mc.Batch(rest), st1.copy())
    e1 = mc.events_by_stream(m1, b1, len(streams))
    e2 = mc.events_by_stream(m2, b2, len(streams))
    for j, s in enumerate(streams):
        assert e1[j] + e2[j] == mc.session_events(s), "stream %d" % j


@pytest.mark.parametrize("group", range(20))
def test_fuzz(codec, group):
    """200 seeds (ten per case): at most 64 frames in at most 16 streams,
    payloads up to 20 KiB, the opcodes of tests/test_gpu_rx_batch.py, masked
    with probability 0.7.  Every third seed also goes through run_damaged
    with a few wire bytes overwritten or the wire cut short."""
    for seed in range(10 * group, 10 * group + 10):
        rng = np.random.default_rng(9000 + seed)
        ns = int(rng.integers(1, 17))
        left = 64
        streams = []
        for _ in range(ns):
            k = int(rng.integers(0, min(left, 12) + 1))
            left -= k
            streams.append(mc.random_frames(rng, k, int(rng.choice([40, 600, 20 * 1024 + 1])), masked_p=0.7))
        batch = mc.Batch(streams)
        run(codec, batch)
        # every third seed, as tests/test_gpu_fuzz.py: one to three wire bytes
        # overwritten, the wire cut short with probability 0.3, the same
        # frame table
        if seed % 3 == 0 and len(batch.wire):
            rng = np.random.default_rng(7000 + seed)
            bad = batch.wire.copy()
            for q in rng.integers(0, len(bad), int(rng.integers(1, 4))):
                bad[q] = rng.integers(0, 256)
            if rng.random() < 0.3:
                bad = bad[: int(rng.integers(0, len(bad)))]
            run_damaged(codec, batch, bad, batch.fs)


def test_round_trip_with_encode_batch(codec):
    """wsg_encode_batch's dense payloads come back from wsg_decode_messages,
    one stream per frame."""
    rng = np.random.default_rng(500)
    lens = np.concatenate([rng.integers(0, 9000, 300), [0, 1, 125, 126, 65535, 65536, 70001]])
    rng.shuffle(lens)
    desc, total = wl.ragged_desc(rng, lens)
    desc["opcode"] = rng.choice([0x81, 0x82], len(lens))
    desc["mask"] = rng.random(len(lens)) < 0.7
    # the sender XORs unmasked frames too (ws.cpp:269-270) and no receiver undoes that: key 0 keeps them plain
    desc["key"][desc["mask"] == 0] = 0
    payload = wl.random_bytes(rng, total)
    n = len(lens)
    cap = int(layout.frame_sizes(desc).sum())
    wire, off = codec.encode_batch(dev(payload), ca.desc_to_tensor(desc, "cuda"), wire_cap=cap)
    assert codec.sync_status() == 0 and int(off[n].item()) == cap
    sf = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    msg = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    msg, msgs, count, state, _ = codec.decode_messages(wire[:cap], off[:n], sf, msg=msg, msg_cap=cap)
    assert codec.sync_status() == 0
    count = count.cpu().numpy()
    assert [int(x) for x in count] == [n, total]
    got = msg.cpu().numpy()
    assert np.array_equal(got[:total], payload) and (got[total:] == SENTINEL).all()
    table = msgs.cpu().numpy().view(MSG)[:n]
    assert np.array_equal(table["off"], desc["src_off"]) and np.array_equal(table["len"], desc["len"])
    assert (table["kind"] == ca.CB_RECEIVED).all()
    assert (state.cpu().numpy().view(STREAM_STATE)["consumed"] == 1).all()


def _raw_call(codec, batch, wire_len=None, msg_cap=None):
    n, ns = batch.n, batch.n_streams
    cap = len(batch.wire) if msg_cap is None else msg_cap
    d_state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    d_msg = torch.full((len(batch.wire) + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    wire = dev(batch.wire)
    _, msgs, count, _, info = codec.decode_messages(wire[: len(batch.wire) if wire_len is None else wire_len],
                                                    dev(batch.fs.view(np.int64)), dev(batch.stream_first),
                                                    state=d_state, msg=d_msg, msg_cap=cap)
    status = codec.sync_status()
    return status, d_msg.cpu().numpy(), count.cpu().numpy(), info


def _frame_bytes(wire, info, k):
    """Frame k's payload unmasked from the wire itself (frames of a garbage
    table may overlap: each is unmasked on its own, as the gather does)."""
    p = wire[int(info["payload_off"][k]):][: int(info["len"][k])]
    kb = np.frombuffer(int(info["key"][k]).to_bytes(4, "little"), np.uint8)
    return p ^ kb[np.arange(len(p)) % 4]


@pytest.mark.parametrize("case", [1, 2, 3, "repeat"])
def test_garbage_frame_table(codec, case):
    """tests/test_gpu_parity.py::test_decode_garbage_starts_match_oracle's
    tables (unsorted, repeated, past the wire's end, pointing into payloads)
    over a whole wire, in a few streams; "repeat": one large FIN frame named
    150 times, so that the payloads overlap and the bytes needed pass
    msg_cap = len(wire).  info equals the oracle's, count the model's; status
    is the oracle's frame error if there is one, else WSG_ENOMEM when
    count[1] > msg_cap, else 0; d_msg holds the model's bytes (need <= cap) or
    is untouched (need > cap), and is never written past msg_cap.  (The table
    and the state are the model's too when the bytes fit.)"""
    if case == "repeat":
        rng = np.random.default_rng(4)
        wire, fs = _frames_wire(rng, rng.integers(0, 3000, 20).astype(np.uint64))
        sizes = np.diff(np.concatenate([fs, [len(wire)]]).astype(np.int64))
        i = int(np.argmax(np.where((wire[fs.astype(np.int64)] & 0x80) != 0, sizes[: len(fs)], -1)[:-1]))
        bad = np.tile(fs[i: i + 2], 150)   # the frame, then the start after it (EINVAL: the next start lies before it)
    else:
        rng = np.random.default_rng(case)
        lens = rng.integers(0, 3000, 300).astype(np.uint64)
        wire, fs = _frames_wire(rng, lens)
        bad = fs.copy()
        pick = rng.random(len(bad))
        bad[pick < 0.2] = rng.integers(0, len(wire) + 100, int((pick < 0.2).sum()))
        bad[(pick >= 0.2) & (pick < 0.25)] = 0
        rng.shuffle(bad[: len(bad) // 3])
    n = len(bad)

    class Table:   # what _call_sentinel reads of a batch
        pass

    batch = Table()
    batch.n, batch.n_streams = n, 5
    batch.stream_first = np.array([0, 40, 40, 150, 299, n], dtype=np.int32)
    cap = len(wire)
    status, count, msg, msgs_all, new_state, info = _call_sentinel(codec, batch, wire, bad, cap)
    rc_o, _, info_o = oracle.decode_batch(wire, bad)
    assert rc_o != 0
    mc.same_fields(info, info_o, mc.INFO_FIELDS)
    want_msgs, want_count, want_state = layout.message_plan(info_o, batch.stream_first, None)
    assert [int(x) for x in count] == [int(x) for x in want_count]
    need = int(count[1])
    assert int(count[0]) > 100 and need > 100000   # whole messages are still delivered
    assert (need > cap) == (case == "repeat")
    assert status == rc_o
    assert (msg[cap:] == SENTINEL).all()
    assert (msgs_all[int(count[0]):].view(np.uint8) == SENTINEL).all()
    if need > cap:
        assert (msg == SENTINEL).all()
        return
    parts = [_frame_bytes(wire, info_o, i) for j in range(batch.n_streams)
             for i in range(int(batch.stream_first[j]), int(batch.stream_first[j]) + int(want_state["consumed"][j]))]
    assert np.array_equal(msg[:need], np.concatenate(parts))
    assert (msg[need:] == SENTINEL).all()
    # a close message's status: the first two bytes of its frames' payloads
    for q in range(len(want_msgs)):
        if int(want_msgs["opcode"][q]) == 8 and int(want_msgs["status"][q]) == 0:   # (1000: fewer than two bytes)
            first = int(want_msgs["first_frame"][q])
            head = np.concatenate([_frame_bytes(wire, info_o, k)[:2]
                                   for k in range(first, first + int(want_msgs["nframes"][q]))])[:2]
            want_msgs["status"][q] = int(head[0]) << 8 | int(head[1])
    mc.same_fields(msgs_all[: int(count[0])], want_msgs, mc.MSG_FIELDS)
    mc.same_fields(new_state, want_state, ["consumed", "opcode"])


def test_latched_truncated_wire(codec):
    rng = np.random.default_rng(600)
    frames = [mc.raw_frame(0x82, rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), key=5 + i) for i in range(9)]
    batch = mc.Batch([frames[:4], frames[4:]])
    status, msg, count, info = _raw_call(codec, batch, wire_len=len(batch.wire) - 100)
    assert status == ca.WSG_ETRUNC
    assert int(ca.info_to_numpy(info, batch.n)["error"][-1]) == ca.WSG_ETRUNC
    assert (msg[len(batch.wire):] == SENTINEL).all()
    assert codec.sync_status() == 0   # the latch is cleared


def test_latched_msg_cap_short(codec):
    rng = np.random.default_rng(601)
    frames = [mc.raw_frame(0x82, rng.integers(0, 256, 700 + i, dtype=np.uint8).tobytes(), key=5 + i) for i in range(9)]
    batch = mc.Batch([frames[:4], frames[4:] + [mc.raw_frame(0x02, b"tail")]])
    need = sum(700 + i for i in range(9))
    status, msg, count, _ = _raw_call(codec, batch, msg_cap=need - 1)
    assert status == ca.WSG_ENOMEM
    assert (msg == SENTINEL).all()                       # no byte of d_msg is written
    assert [int(x) for x in count] == [9, need]          # ... and the caller can size a retry
    status, msg, count, _ = _raw_call(codec, batch, msg_cap=need)
    assert status == 0 and (msg[need:] == SENTINEL).all() and not (msg[:need] == SENTINEL).all()


def test_checked_launch_refuses_short_msgs_table():
    """$WSG_CHECK=1 in a fresh process (tests/messages_check_job.py): a d_msgs
    block one record short is WSG_EINVAL and nothing is launched."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    job = os.path.join(root, "tests", "messages_check_job.py")
    r = subprocess.run([sys.executable, job], env=dict(os.environ, WSG_CHECK="1"), capture_output=True, text=True,
                       timeout=90, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"], json.dumps(res)
