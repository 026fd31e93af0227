"""The device entry points driven asynchronously, against the oracle.

wsg_capi.h promises that wsg_decode_batch, wsg_decode_messages,
wsg_encode_batch and the fan-out calls are asynchronous on the caller's
stream.  The other GPU files make one call on torch's current stream and
synchronise; here the calls are driven the three ways a server drives them:

  A  a chain of calls on one side stream with no host synchronisation, later
     calls reading earlier calls' outputs (and their device frame tables)
     straight from HBM and reusing the context's scratch under other layouts,
     a scratch regrow in the middle;
  B  the error latch over such a chain (wsg_sync reports the error of the
     lowest frame index over all the calls since the last wsg_sync);
  C  two streams on one context: wsg_encode_batch calls share one scratch and
     wsg_decode_messages calls another, and the library orders them on the
     device (an event behind each call, hipStreamWaitEvent before the next one
     on another stream);
  D  the launches captured into a HIP graph and replayed over new inputs.

Every expected byte is the oracle's; every device output lies in a buffer
filled with 0xA5 and the bytes behind it must still hold that.  Bit-exact.
"""
import functools
import time

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout, workloads as wl  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, SEND_DESC, STREAM_STATE, frame_size  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests.test_gpu_parity import INFO_FIELDS, SMALL_AVG, _mixed_desc  # noqa: E402

SENTINEL = 0xA5
PAD = 4096              # sentinel bytes behind every output
SCAN_ITEMS = 1024       # wsg_internal.h: frames of one encode scan block

# torch.cuda._sleep cycles of the kernel that holds both streams back while
# the two-stream tests queue their rounds (test C).  Measured on an MI355X:
# _sleep(1e8) lasts 41.9 ms (2.4 cycles per ns); queueing 32 rounds x 2
# encodes takes the host 1.0-1.3 ms (piece/piece 1.27, small/small 0.95-1.01),
# 16 rounds x 2 decode_messages 1.1 ms.  5e7 cycles = 21 ms: 16 times the
# slowest loop (3 times is the least a run should have).
GATE_CYCLES = 50_000_000


@pytest.fixture()
def codec():
    """A fresh context for every test."""
    c = ca.Codec(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sent(nbytes):
    return torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device="cuda")


def tail_kept(buf, used):
    return bool((buf[int(used):] == SENTINEL).all())


# ------------------------------------------------------------ operands, checks
class EncOut:
    """Outputs of one wsg_encode_batch call: the wire (room bytes + PAD) and
    the n + 1 offsets (+ PAD), sentinel-filled."""

    def __init__(self, n, room):
        self.n = n
        self.wire = sent(room + PAD)
        self.offb = sent((n + 1) * 8 + PAD)
        self.off = self.offb[: (n + 1) * 8].view(torch.int64)

    def refill(self):
        self.wire.fill_(SENTINEL)
        self.offb.fill_(SENTINEL)

    def check(self, ref):
        """Offsets and bytes against oracle.encode_batch's; the sentinel behind both."""
        wire_o, off_o = ref
        total = int(off_o[self.n])
        assert np.array_equal(self.off.cpu().numpy().view(np.uint64), off_o)
        assert tail_kept(self.offb, (self.n + 1) * 8), "offsets written past n + 1"
        assert np.array_equal(self.wire[:total].cpu().numpy(), wire_o)
        assert tail_kept(self.wire, total), "bytes written past the last frame"


def encode(codec, p, d, out, cap, stream=None):
    codec.encode_batch(p, d, wire=out.wire, wire_cap=cap, wire_off=out.off, stream=stream)


class DecOut:
    """Outputs of one wsg_decode_batch call of nbytes of wire and n frames."""

    def __init__(self, nbytes, n):
        self.nbytes, self.n = nbytes, n
        self.buf = sent(nbytes + PAD)
        self.out = self.buf[:nbytes]
        self.info = sent(n * RECV_INFO.itemsize + PAD)

    def refill(self):
        self.buf.fill_(SENTINEL)
        self.info.fill_(SENTINEL)

    def check(self, ref):
        """Bytes and records against oracle.decode_batch's (rc, out, info)."""
        _, out_o, info_o = ref
        assert np.array_equal(self.out.cpu().numpy(), out_o)
        assert tail_kept(self.buf, self.nbytes), "bytes written past wire_len"
        got = ca.info_to_numpy(self.info, self.n)
        for f in INFO_FIELDS:
            assert np.array_equal(got[f], info_o[f]), f
        assert tail_kept(self.info, self.n * RECV_INFO.itemsize), "records written past frame n"
        return got


class MsgWant:
    """What wsg_decode_messages must make of a messages_cases.Batch: the
    oracle's records, layout.message_plan over them, the dense bytes."""

    def __init__(self, batch):
        self.batch = batch
        self.out, self.info = batch.oracle_decode()
        self.msgs, self.count, self.state = layout.message_plan(self.info, batch.stream_first, None, payload=self.out)
        self.bytes = mc.dense(self.out, self.info, batch.stream_first, self.state)


class MsgOut:
    """Outputs of one wsg_decode_messages call (n frames, ns streams, msg_cap
    bytes of messages), each with PAD sentinel bytes behind it."""

    def __init__(self, n, ns, cap):
        self.n, self.ns, self.cap = n, ns, cap
        st = np.full(ns * STREAM_STATE.itemsize + PAD, SENTINEL, dtype=np.uint8)
        st[: ns * STREAM_STATE.itemsize].view(STREAM_STATE)["opcode"] = 0   # the seed: no message open
        self.state = dev(st)
        self.msg = sent(cap + PAD)
        self.msgs = sent(n * MSG.itemsize + PAD)
        self.count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.info = sent(n * RECV_INFO.itemsize + PAD)

    def check(self, want, events=True):
        """Counts, table, state, records and bytes against `want`; the
        sentinel behind each; with `events` the callbacks against one oracle
        session per stream (messages_cases.check_events)."""
        n, ns = self.n, self.ns
        count = [int(x) for x in self.count.cpu().numpy()]
        assert count == [int(x) for x in want.count]
        info = ca.info_to_numpy(self.info, n)
        mc.same_fields(info, want.info, mc.INFO_FIELDS)
        assert tail_kept(self.info, n * RECV_INFO.itemsize)
        table = self.msgs.cpu().numpy()
        msgs = table[: count[0] * MSG.itemsize].view(MSG)
        mc.same_fields(msgs, want.msgs, mc.MSG_FIELDS)
        assert (table[count[0] * MSG.itemsize:] == SENTINEL).all(), "records written past count[0]"
        st = self.state.cpu().numpy()
        state = st[: ns * STREAM_STATE.itemsize].view(STREAM_STATE)
        mc.same_fields(state, want.state, ["consumed", "opcode"])
        assert (st[ns * STREAM_STATE.itemsize:] == SENTINEL).all(), "states written past n_streams"
        msg = self.msg.cpu().numpy()
        assert np.array_equal(msg[: count[1]], want.bytes)
        assert (msg[count[1]:] == SENTINEL).all(), "bytes written past count[1]"
        if events:
            mc.check_events(want.batch, msgs, msg[: count[1]], state, want.info, None)


def decode_messages(codec, wire, fs, stream_first, o, stream=None):
    codec.decode_messages(wire, fs, stream_first, state=o.state[: o.ns * STREAM_STATE.itemsize], msg=o.msg,
                          msg_cap=o.cap, msgs=o.msgs, count=o.count, info=o.info, stream=stream)


def fanout_room(length, k):
    return frame_size(0x82, True, length) * k


def check_fanout(buf, ref):
    got = buf.cpu().numpy()
    assert np.array_equal(got[: len(ref)], ref)
    assert (got[len(ref):] == SENTINEL).all(), "bytes written past the last frame"


def batch_of(wire, off, cuts):
    """The frames of an encoded wire as a messages_cases.Batch whose stream j
    holds frames [cuts[j], cuts[j + 1])."""
    frames = [wire[int(off[i]): int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
    b = mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(len(cuts) - 1)])
    assert np.array_equal(b.wire, wire) and np.array_equal(b.fs, off[:-1])
    return b


# ------------------------------------------- A. the chain, no host sync inside
FAN_PERIOD = (4096, 1000)   # payload bytes x keys: the period kernel
FAN_FLAT = (1010, 700)      # ... the flat kernel
N_BIG, N_SMALL, N_GROW = 300, 3000, 40000
MSG_STREAMS = 7


@functools.lru_cache(maxsize=None)
def _chain():
    """The chain's inputs and the oracle's result of every call, computed once."""
    rng = np.random.default_rng(501)
    c = {}
    c["p1"], c["d1"] = _mixed_desc(rng, N_BIG, 100, 70000)
    c["ref1"] = oracle.encode_batch(c["p1"], c["d1"])
    c["p2"], c["d2"] = _mixed_desc(rng, N_SMALL, 0, 40)
    c["ref2"] = oracle.encode_batch(c["p2"], c["d2"])
    wire1, off1 = c["ref1"]
    c["dec1"] = oracle.decode_batch(wire1, off1[:-1])
    assert c["dec1"][0] == 0
    cuts = np.concatenate([[0], np.sort(rng.integers(0, N_SMALL + 1, MSG_STREAMS - 1)), [N_SMALL]])
    cuts[3] = cuts[2]   # an empty stream among the seven
    cuts.sort()
    c["want2"] = MsgWant(batch_of(*c["ref2"], [int(x) for x in cuts]))
    for name, (length, k), seed in (("fan_p", FAN_PERIOD, 61), ("fan_f", FAN_FLAT, 62)):
        payload, keys = wl.c4_fanout(length, k, seed=seed)
        c[name] = (payload, keys, oracle.fanout_encode(payload, keys, 0x82, True))
    c["p6"], c["d6"] = _mixed_desc(rng, N_GROW, 0, 40)
    c["ref6"] = oracle.encode_batch(c["p6"], c["d6"])
    return c


@pytest.mark.parametrize("which", ["side", "own"])
def test_chain_without_host_sync(codec, which):
    """Ten calls queued back to back on one stream (a torch side stream; the
    context's own wsg_stream), one wsg_sync at the end:
      1  piece-path encode, 300 frames of 100-70 000 B
      2  small-path encode, 3 000 frames of 0-40 B at exact capacity: the
         scratch of call 1 under the other layout
      3  decode_batch of call 1's wire with call 1's device offsets as the
         frame table, out of place; then in place on a device copy
      4  decode_messages of call 2's wire (7 streams, call 2's device offsets)
      5  a period-path and a flat-path fan-out
      6  a 40 000-frame small-path encode: the first n above 32 768, so the
         piece-start scratch grows (the library synchronises the device for
         that, between the calls still pending and the next one), then call 1
         again into other outputs.
    Buffers are made and filled on the default stream and the device
    synchronised before the first call; nothing but the library's calls and
    one device copy happens on the stream until the sync."""
    c = _chain()
    total1, total2, total6 = (int(c[k][1][-1]) for k in ("ref1", "ref2", "ref6"))
    cap1 = max(total1, N_BIG * SMALL_AVG + 4096)
    assert cap1 > N_BIG * SMALL_AVG and total2 <= N_SMALL * SMALL_AVG and total6 <= N_GROW * SMALL_AVG
    assert N_GROW > 32768 >= max(N_BIG, N_SMALL)
    want2 = c["want2"]

    p1, d1 = dev(c["p1"]), ca.desc_to_tensor(c["d1"], "cuda")
    p2, d2 = dev(c["p2"]), ca.desc_to_tensor(c["d2"], "cuda")
    p6, d6 = dev(c["p6"]), ca.desc_to_tensor(c["d6"], "cuda")
    e1, e1b = EncOut(N_BIG, cap1), EncOut(N_BIG, cap1)
    e2, e6 = EncOut(N_SMALL, total2), EncOut(N_GROW, total6)
    dec_a, dec_b = DecOut(total1, N_BIG), DecOut(total1, N_BIG)
    m4 = MsgOut(N_SMALL, MSG_STREAMS, total2)
    sf = dev(want2.batch.stream_first)
    fans = []
    for name, (length, k) in (("fan_p", FAN_PERIOD), ("fan_f", FAN_FLAT)):
        payload, keys, ref = c[name]
        assert len(ref) == fanout_room(length, k)
        buf = sent(len(ref) + PAD)
        fans.append((dev(payload), dev(keys.view(np.int32)), buf, ref))
    torch.cuda.synchronize()

    st = torch.cuda.Stream() if which == "side" else codec.own_stream()
    assert st.cuda_stream != torch.cuda.default_stream().cuda_stream
    if which == "own":
        assert st.cuda_stream == ca.lib().wsg_stream(codec._ctx)
    encode(codec, p1, d1, e1, cap1, st)                                          # 1
    encode(codec, p2, d2, e2, total2, st)                                        # 2
    codec.decode_batch(e1.wire[:total1], e1.off[:-1], out=dec_a.out, info=dec_a.info, stream=st)   # 3
    with torch.cuda.stream(st):
        dec_b.out.copy_(e1.wire[:total1])
    codec.decode_batch(dec_b.out, e1.off[:-1], out=dec_b.out, info=dec_b.info, stream=st)
    decode_messages(codec, e2.wire[:total2], e2.off[:-1], sf, m4, st)            # 4
    for payload, keys, buf, ref in fans:                                         # 5
        codec.fanout(payload, keys, 0x82, True, wire=buf[: len(ref)], stream=st)
    encode(codec, p6, d6, e6, total6, st)                                        # 6
    encode(codec, p1, d1, e1b, cap1, st)
    codec.sync(st)

    e1.check(c["ref1"])
    e2.check(c["ref2"])
    dec_a.check(c["dec1"])
    dec_b.check(c["dec1"])
    m4.check(want2)
    for _, _, buf, ref in fans:
        check_fanout(buf, ref)
    e6.check(c["ref6"])
    e1b.check(c["ref1"])
    assert codec.sync_status(st) == 0


# ------------------------------------------------------- B. the error latch
@pytest.mark.parametrize("third", ["clean", "one-byte-short"])
def test_error_latch_over_unsynchronised_calls(codec, third):
    """On a side stream, no sync between: a decode whose last frame is cut
    short (WSG_ETRUNC at frame 39), a clean decode of another wire, an
    encode.  One wsg_sync returns the error and clears the latch; the clean
    calls' results are untouched by it, and the cut decode's bytes and
    records are the oracle's for that wire.
    one-byte-short: the third call encodes one frame into a capacity one
    byte short, which latches WSG_ENOMEM at frame 0: the latch keeps the
    minimum of frame << 8 | code, so the sync reports that error, of the
    lowest frame index over the three calls, not the one latched first."""
    rng = np.random.default_rng(601 + len(third))
    n = 40
    lens = rng.integers(0, 3000, n)
    lens[-1] = 500
    p, d = _desc_of(rng, lens)
    wire_t, off_t = oracle.encode_batch(p, d)
    cut = wire_t[: len(wire_t) - 3]
    fs_t = off_t[:-1]
    ref_t = oracle.decode_batch(cut, fs_t)
    assert ref_t[0] == ca.WSG_ETRUNC
    assert list(np.nonzero(ref_t[2]["error"])[0]) == [n - 1] and int(ref_t[2]["error"][n - 1]) == ca.WSG_ETRUNC
    p, d = _mixed_desc(rng, 500, 0, 2000)
    wire_c, off_c = oracle.encode_batch(p, d)
    ref_c = oracle.decode_batch(wire_c, off_c[:-1])
    assert ref_c[0] == 0
    ne = 1 if third == "one-byte-short" else 700
    pe, de = _mixed_desc(rng, ne, 10, 900)
    ref_e = oracle.encode_batch(pe, de)
    total_e = int(ref_e[1][-1])
    cap_e = total_e - 1 if third == "one-byte-short" else total_e

    w_t, f_t, o_t = dev(cut), dev(fs_t.view(np.int64)), DecOut(len(cut), n)
    w_c, f_c, o_c = dev(wire_c), dev(off_c[:-1].view(np.int64)), DecOut(len(wire_c), 500)
    d_pe, d_de, o_e = dev(pe), ca.desc_to_tensor(de, "cuda"), EncOut(ne, total_e)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    codec.decode_batch(w_t, f_t, out=o_t.out, info=o_t.info, stream=st)
    codec.decode_batch(w_c, f_c, out=o_c.out, info=o_c.info, stream=st)
    encode(codec, d_pe, d_de, o_e, cap_e, st)
    assert codec.sync_status(st) == (ca.WSG_ENOMEM if third == "one-byte-short" else ca.WSG_ETRUNC)
    assert codec.sync_status(st) == 0

    got = o_c.check(ref_c)
    assert not got["error"].any()
    o_t.check(ref_t)
    if third == "clean":
        o_e.check(ref_e)
    else:   # the offsets are final, no frame byte is written
        assert np.array_equal(o_e.off.cpu().numpy().view(np.uint64), ref_e[1])
        assert tail_kept(o_e.wire, 0) and tail_kept(o_e.offb, (ne + 1) * 8)


# ------------------------------------------------ C. two streams, one context
def _gate(streams):
    """Hold `streams` back behind a sleeping kernel on a third stream; returns
    the event that fires when it ends."""
    s0 = torch.cuda.Stream()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s0):
        torch.cuda._sleep(GATE_CYCLES)
        ev.record(s0)
    for s in streams:
        s.wait_event(ev)
    return ev


def _desc_of(rng, lens):
    """_mixed_desc's frames with these payload lengths."""
    n = len(lens)
    desc, total = wl.ragged_desc(rng, lens)
    desc["opcode"] = rng.choice([0x81, 0x82, 0x01, 0x02, 0x00, 0x80, 0x88, 0x89, 0x8A, 0xC2, 0x83], n)
    desc["mask"] = rng.random(n) < 0.6
    desc["status"] = np.where(rng.random(n) < 0.3, rng.integers(-5, 70000, n), 0)
    desc["src_off"] += rng.integers(0, 16, n).astype(np.uint64)
    return wl.random_bytes(rng, total + 16), desc


N_TWO = 4096
ROUNDS_ENC, ROUNDS_MSG = 32, 16


@functools.lru_cache(maxsize=None)
def _two_batches():
    """A: lengths uniform 0-4000; B: the same from another seed, sorted
    descending.  The scan-block sums and most frame offsets differ, or a mixed
    scratch would give the right bytes all the same."""
    ra, rb = np.random.default_rng(701), np.random.default_rng(702)
    pa, da = _desc_of(ra, ra.integers(0, 4001, N_TWO))
    pb, db = _desc_of(rb, np.sort(rb.integers(0, 4001, N_TWO))[::-1])
    sa, sb = ca.frame_sizes(da), ca.frame_sizes(db)
    groups_a = sa.reshape(-1, SCAN_ITEMS).sum(axis=1)
    groups_b = sb.reshape(-1, SCAN_ITEMS).sum(axis=1)
    assert (groups_a != groups_b).all()
    assert int((np.cumsum(sa)[:-1] != np.cumsum(sb)[:-1]).sum()) > N_TWO // 2
    return (pa, da, oracle.encode_batch(pa, da)), (pb, db, oracle.encode_batch(pb, db))


def _pieces(desc):
    """The piece kernel's count for these frames (pieces_of, wsg_encode.hip)."""
    return int(((ca.frame_sizes(desc) + np.uint64(127 + 4095)) // np.uint64(4096)).sum())


CAP_PIECE, CAP_SMALL = N_TWO * SMALL_AVG + 4096, N_TWO * SMALL_AVG


@pytest.fixture(scope="module")
def shared_codec():
    """The one context of the two-stream tests."""
    c = ca.Codec(0)
    yield c
    c.close()


@pytest.mark.parametrize("pair", ["piece-piece", "small-small", "piece-small"])
def test_two_streams_encode(shared_codec, pair):
    """32 rounds of (encode A on S1, encode B on S2) on one context, all
    queued while a sleeping kernel holds both streams back, every round into
    outputs of its own.  Both calls use the context's encode scratch: the
    library runs them one after the other on the device.  The pairs: both on
    the piece kernels (wire_cap n * 4096 + 4096), both on the small-frame
    kernel (n * 4096), A on the piece kernels and B on the small-frame one
    (equal n, so those two capacities).  Every wire tensor has room for
    capA + capB + 4096 bytes: with equal n and a warmed scratch, offsets
    made from a mixture of the two calls' scratch stay below totalA + totalB.
    (One run on the library before the calls were ordered: piece-piece right,
    small-small 3 of 64 calls wrong, piece-small 1 of 64, all in rounds 0-1.)"""
    codec = shared_codec
    (pa, da, ref_a), (pb, db, ref_b) = _two_batches()
    cap_a = CAP_SMALL if pair == "small-small" else CAP_PIECE
    cap_b = CAP_PIECE if pair == "piece-piece" else CAP_SMALL
    total_a, total_b = int(ref_a[1][-1]), int(ref_b[1][-1])
    assert max(total_a, total_b) <= CAP_SMALL
    room = cap_a + cap_b + 4096
    d_pa, d_da = dev(pa), ca.desc_to_tensor(da, "cuda")
    d_pb, d_db = dev(pb), ca.desc_to_tensor(db, "cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    # the scratch sized and every entry a later call may read initialised:
    # one synchronised call of the batch with more pieces, at the larger capacity
    first = (d_pa, d_da, ref_a) if _pieces(da) >= _pieces(db) else (d_pb, d_db, ref_b)
    warm = EncOut(N_TWO, room)
    encode(codec, first[0], first[1], warm, max(cap_a, cap_b))
    assert codec.sync_status() == 0
    warm.check(first[2])

    outs = [(EncOut(N_TWO, room), EncOut(N_TWO, room)) for _ in range(ROUNDS_ENC)]
    want = [(dev(ref[0]), dev(ref[1].view(np.int64))) for ref in (ref_a, ref_b)]
    torch.cuda.synchronize()
    gate = _gate([s1, s2])
    t0 = time.perf_counter()
    for oa, ob in outs:
        encode(codec, d_pa, d_da, oa, cap_a, s1)
        encode(codec, d_pb, d_db, ob, cap_b, s2)
    queued = time.perf_counter() - t0
    opened = gate.query()
    print("two-stream encode %s: %d rounds queued in %.2f ms" % (pair, ROUNDS_ENC, queued * 1e3))
    assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
    torch.cuda.synchronize()
    assert not opened, "the gate opened before every call was queued (%.2f ms)" % (queued * 1e3)

    bad = []
    for r, pair_out in enumerate(outs):
        for o, (w, off), total, name in zip(pair_out, want, (total_a, total_b), "AB"):
            ok = (torch.equal(o.off, off) and torch.equal(o.wire[:total], w) and tail_kept(o.wire, total)
                  and tail_kept(o.offb, (N_TWO + 1) * 8))
            if not ok:
                bad.append("%d%s" % (r, name))
    assert not bad, "%d of %d calls wrong (round, batch): %s" % (len(bad), 2 * ROUNDS_ENC, " ".join(bad))


@functools.lru_cache(maxsize=None)
def _two_message_batches():
    """Two batches of the same frames in another order over other stream
    boundaries: wire_len, n, n_streams and msg_cap agree, the geometry not."""
    rng = np.random.default_rng(801)
    n, ns = 2000, 8
    frames = mc.random_frames(rng, n, 3000)
    wants = []
    for k in range(2):
        order = np.arange(n) if k == 0 else rng.permutation(n)
        cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, ns - 1)), [n]])
        fr = [frames[i] for i in order]
        wants.append(MsgWant(mc.Batch([fr[cuts[j]: cuts[j + 1]] for j in range(ns)])))
    a, b = wants
    assert len(a.batch.wire) == len(b.batch.wire) and a.batch.n == b.batch.n == n
    assert int((a.batch.fs != b.batch.fs).sum()) > n // 2
    assert int(a.count[0]) != int(b.count[0]) or not np.array_equal(a.msgs["len"], b.msgs["len"])
    return a, b


def test_two_streams_decode_messages(shared_codec):
    """The same for wsg_decode_messages, whose plan block and piece records
    are the context's: 16 rounds of (batch A on S1, batch B on S2) queued
    behind the gate, every result against the oracle (the callbacks of the
    first round's against the sessions)."""
    codec = shared_codec
    wants = _two_message_batches()
    n, ns, wire_len = wants[0].batch.n, wants[0].batch.n_streams, len(wants[0].batch.wire)
    ins = []
    for w in wants:
        buf = sent(2 * wire_len + 4096)
        buf[:wire_len].copy_(torch.from_numpy(w.batch.wire))
        ins.append((buf[:wire_len], dev(w.batch.fs.view(np.int64)), dev(w.batch.stream_first)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for w, i in zip(wants, ins):   # sized, and each batch checked on its own
        o = MsgOut(n, ns, wire_len)
        decode_messages(codec, *i, o)
        assert codec.sync_status() == 0
        o.check(w)
    outs = [(MsgOut(n, ns, wire_len), MsgOut(n, ns, wire_len)) for _ in range(ROUNDS_MSG)]
    torch.cuda.synchronize()
    gate = _gate([s1, s2])
    t0 = time.perf_counter()
    for oa, ob in outs:
        decode_messages(codec, *ins[0], oa, s1)
        decode_messages(codec, *ins[1], ob, s2)
    queued = time.perf_counter() - t0
    opened = gate.query()
    print("two-stream decode_messages: %d rounds queued in %.2f ms" % (ROUNDS_MSG, queued * 1e3))
    assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
    torch.cuda.synchronize()
    assert not opened, "the gate opened before every call was queued (%.2f ms)" % (queued * 1e3)
    for r, pair_out in enumerate(outs):
        for o, w in zip(pair_out, wants):
            o.check(w, events=r == 0)


# ------------------------------------------------------------ D. graph replay
N_GRAPH = 2048
GRAPH_CAP_PIECE, GRAPH_CAP_SMALL = N_GRAPH * SMALL_AVG + 4096, N_GRAPH * 64
GRAPH_PAYLOAD = N_GRAPH * 7000 + 32


def _decode_wire(rng, lens, mask):
    """Frames of these payload lengths and mask bits with new keys, opcodes
    and bytes: the frame table depends on `lens` and `mask` alone."""
    n = len(lens)
    desc = np.zeros(n, dtype=SEND_DESC)
    desc["len"] = lens
    desc["mask"] = mask
    desc["key"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    desc["opcode"] = rng.choice([0x81, 0x82, 0x01, 0x02, 0x00, 0x80], n)   # no status prefix: it would add bytes
    payload = wl.random_bytes(rng, int(lens.max()) + 16)
    desc["src_off"] = rng.integers(0, 16, n)
    wire, off = oracle.encode_batch(payload, desc)
    return wire, off[:-1].copy()


def test_graph_replay(codec):
    """A period and a flat fan-out, a decode whose tiles take the stream, the
    boundary and the staged path, a piece-path and a small-path encode
    captured into one graph on a side stream, each call run once before so
    that nothing allocates under capture.  Five replays, each after new
    payloads, keys, descriptors and decode wire (same frame lengths) were
    written into the captured buffers and the outputs refilled with the
    sentinel: every output against the oracle.  In the fourth the decode
    wire's last frame claims more bytes than the wire holds: wsg_sync returns
    WSG_ETRUNC, everything else is still right, and the fifth returns 0."""
    seeds = np.random.default_rng(901)
    fixed = np.random.default_rng(902)
    lens = fixed.choice([0, 0, 0, 1, 5, 300, 20000], 1500).astype(np.uint64)
    lens[-1] = 5
    mask = fixed.random(1500) < 0.6
    fs0 = None

    def inputs(truncate):
        nonlocal fs0
        rng = np.random.default_rng(int(seeds.integers(0, 2**31)))
        x = {}
        for name, (length, k) in (("fan_p", FAN_PERIOD), ("fan_f", FAN_FLAT)):
            payload, keys = wl.c4_fanout(length, k, seed=int(rng.integers(0, 2**31)))
            x[name] = (payload, keys, oracle.fanout_encode(payload, keys, 0x82, True))
        wire, fs = _decode_wire(rng, lens, mask)
        if fs0 is None:
            fs0 = fs
        assert np.array_equal(fs, fs0)
        if truncate:   # the 7-bit length field of the last frame: 5 -> 100, past the wire's end
            wire = wire.copy()
            assert wire[int(fs[-1]) + 1] & 0x7F == 5
            wire[int(fs[-1]) + 1] = (wire[int(fs[-1]) + 1] & 0x80) | 100
        x["dec"] = (wire, oracle.decode_batch(wire, fs))
        assert x["dec"][1][0] == (ca.WSG_ETRUNC if truncate else 0)
        pp, dp = _mixed_desc(rng, N_GRAPH, 100, 7000)
        ps, ds = _mixed_desc(rng, N_GRAPH, 0, 40)
        x["enc_p"] = (pp, dp, oracle.encode_batch(pp, dp))
        x["enc_s"] = (ps, ds, oracle.encode_batch(ps, ds))
        assert N_GRAPH * SMALL_AVG < GRAPH_CAP_PIECE and int(x["enc_p"][2][1][-1]) <= GRAPH_CAP_PIECE
        assert int(x["enc_s"][2][1][-1]) <= GRAPH_CAP_SMALL <= N_GRAPH * SMALL_AVG
        assert len(pp) <= GRAPH_PAYLOAD and len(ps) <= GRAPH_PAYLOAD
        return x

    x = inputs(False)
    wire_len = len(x["dec"][0])
    # frame starts inside each full 16 KiB tile: none (the stream path), a few
    # (at most 4 frames touch the tile: the boundary path), more (the staged path)
    starts = np.diff(np.searchsorted(fs0, np.arange(0, wire_len, 16384)))
    assert (starts == 0).any() and ((starts >= 1) & (starts <= 3)).any() and (starts >= 5).any()

    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fan = {}
        for name, (length, k) in (("fan_p", FAN_PERIOD), ("fan_f", FAN_FLAT)):
            buf = sent(fanout_room(length, k) + PAD)
            fan[name] = (torch.zeros(length, dtype=torch.uint8, device="cuda"),
                         torch.zeros(k, dtype=torch.int32, device="cuda"), buf)
        d_wire = torch.zeros(wire_len + 16, dtype=torch.uint8, device="cuda")[:wire_len]
        d_fs = dev(fs0.view(np.int64))
        dec = DecOut(wire_len, len(fs0))
        enc = {}
        for name, cap in (("enc_p", GRAPH_CAP_PIECE), ("enc_s", GRAPH_CAP_SMALL)):
            enc[name] = (torch.zeros(GRAPH_PAYLOAD, dtype=torch.uint8, device="cuda"),
                         torch.zeros(N_GRAPH * SEND_DESC.itemsize, dtype=torch.uint8, device="cuda"),
                         EncOut(N_GRAPH, cap), cap)

        def upload(x):
            for name in fan:
                fan[name][0].copy_(torch.from_numpy(x[name][0]))
                fan[name][1].copy_(torch.from_numpy(x[name][1].view(np.int32)))
                fan[name][2].fill_(SENTINEL)
            d_wire.copy_(torch.from_numpy(x["dec"][0]))
            dec.refill()
            for name in enc:
                payload, desc = x[name][0], x[name][1]
                enc[name][0][: len(payload)].copy_(torch.from_numpy(payload))
                enc[name][1].copy_(torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)))
                enc[name][2].refill()

        launches = [codec.prepare_fanout(fan[name][0], fan[name][1], 0x82, True,
                                         fan[name][2][: fanout_room(*geom)])
                    for name, geom in (("fan_p", FAN_PERIOD), ("fan_f", FAN_FLAT))]
        launches.append(codec.prepare_decode(d_wire, d_fs, dec.out, dec.info))

        def calls():
            for launch in launches:
                launch()
            for name in ("enc_p", "enc_s"):
                p, d, o, cap = enc[name]
                encode(codec, p, d, o, cap)

        def check(x, status):
            assert codec.sync_status(st) == status
            for name in fan:
                check_fanout(fan[name][2], x[name][2])
            dec.check(x["dec"][1])
            for name in enc:
                enc[name][2].check(x[name][2])

        upload(x)
        calls()          # every call once, same n and capacity: the scratch is sized
        check(x, 0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            calls()
        for replay in range(5):
            x = inputs(truncate=replay == 3)
            upload(x)
            g.replay()
            check(x, ca.WSG_ETRUNC if replay == 3 else 0)
            assert codec.sync_status(st) == 0
