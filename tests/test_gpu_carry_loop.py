"""The validating echo server's loop with the wire resident on the device.

tests/test_gpu_validated_loop.py's loop of cut reads, but the host never
joins or uploads a wire: a round is one upload of the bytes just read and of
the read table, one wsg_carry_streams into the other of two wire buffers, one
wsg_reply_validated_streams on what it wrote and one wsg_sync.  The wires,
d_state, d_proto, the span tables and d_close_off stay on the device from
round to round; the host reads replies, verdicts and counts.  Stream j is
connection j for good (tests/carry_cases.py::drive).

Every run must pass the checks of the loop it replaces, equal the run of the
same driver over layout.carry_plan and the model's step, and upload exactly
the bytes that were read, fewer than a loop that uploads every round's wire.
Under WSG_ASSEMBLY_RFC the connections, the model's step and the checks are
tests/rfc_assembly_cases.py's, as in tests/test_gpu_rfc_loop.py: there the
carry has to leave d_state[j].ahead working.  Then the reconnect storm of
tests/test_gpu_upgrade_loop.py: wsg_upgrade_streams, the frames of the
accepted connections in the same round, one carry with the rejected ones
dropped."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import PROTO_STATE, PROTO_VERDICT, STREAM_READ, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import carry_cases as kc  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests import test_gpu_validated_reply as vg  # noqa: E402
from tests.test_gpu_server_loop import SCHEDULES  # noqa: E402
from tests.test_gpu_upgrade_loop import BAD, N, request_of  # noqa: E402
from tests.test_gpu_validated_loop import VALIDATING  # noqa: E402

SENTINEL, SENT64, EXTRA = cg.SENTINEL, cg.SENT64, cg.EXTRA
dev, sent = cg.dev, cg.sent
ROOM = 2 << 20   # bytes of each wire buffer (server_loop_cases.WIRE_MAX is half of it)


class Resident:
    """What the loop keeps on the device: two wire buffers and two span
    tables, taken in turns, d_state, d_proto, the last round's d_close_off.
    ``carry`` and ``step`` are the two callables of carry_cases.drive."""

    def __init__(self, codec, n, frame_cap, rule, mask, limit, which, keys, carries):
        self.codec, self.n, self.frame_cap = codec, n, frame_cap
        self.rule, self.mask, self.limit, self.which, self.carries = rule, mask, limit, which, carries
        self.wires = [torch.empty(ROOM + 16, dtype=torch.uint8, device="cuda")[:ROOM] for _ in range(2)]
        self.spans = [torch.zeros(n * STREAM_SPAN.itemsize, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.state = torch.zeros(n * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.proto = torch.zeros(n * PROTO_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.count = sent((4 + EXTRA) * 8).view(torch.int64)
        self.keys = cg.d_keys_of(keys)
        self.turn = 0
        self.uploaded = self.wire_bytes = self.carried = 0

    def carry(self, wire, spans, close_off, new, reads):
        first = isinstance(spans, np.ndarray)   # the first round: no wire, a zeroed table (spans[2] stays zero)
        self.turn ^= 1
        d_new = torch.empty(len(new) + 32, dtype=torch.uint8, device="cuda")[: len(new)]
        d_new.copy_(torch.from_numpy(new))
        self.uploaded += len(new)
        out = self.codec.carry_streams(None if first else wire, self.spans[2] if first else spans, d_new,
                                       dev(reads.view(np.uint8)), close_off=None if first else close_off,
                                       next=self.wires[self.turn], next_cap=ROOM, next_spans=self.spans[self.turn],
                                       count=self.count)
        return out[0], out[1]

    def step(self, wire, spans, state, proto, keys, frame_cap):
        """One wsg_reply_validated_streams over the carry's output (the whole
        buffer as the wire: nothing behind d_count[0] is inside a span) and
        one wsg_sync; d_state and d_proto are the loop's own."""
        n, cap = self.n, ROOM + 14 * self.frame_cap
        o = vg.Out(self.frame_cap, n, cap)
        fs = sent((self.frame_cap + EXTRA) * 8).view(torch.int64)
        sf = sent((n + 1 + EXTRA) * 4).view(torch.int32)
        out = self.codec.reply_validated_streams(
            wire, spans, proto=self.proto, role=pc.SERVER, max_message=self.limit, which=self.which, reply_op=self.rule,
            mask=self.mask, send_keys=self.keys, state=self.state, frame_start=fs, frame_cap=self.frame_cap,
            stream_first=sf, reply=o.reply, reply_cap=cap, reply_off=o.reply_off, stream_reply=o.stream_reply,
            close_off=o.close_off, verdict=o.verdict, result=o.result, valid=o.valid, utf8_result=o.utf8_result,
            msgs=o.msgs, count=o.count, info=o.info)
        assert self.codec.sync_status() == 0
        cnt = self.count.cpu().numpy().view(np.uint64)
        assert (cnt[4:] == SENT64).all() and int(cnt[0]) <= ROOM
        self.wire_bytes += int(cnt[0])
        self.carried += int(cnt[1])
        rcount = o.count.cpu().numpy().view(np.uint64)
        need = int(rcount[2])
        reply = o.reply.cpu().numpy()
        assert out[-1] <= self.frame_cap and need <= cap and (reply[need:] == SENTINEL).all()
        r = sl.Step()
        r.reply, r.stream_reply = reply[:need], o.stream_reply.cpu().numpy().view(np.uint64)
        r.close_off = o.close_off.cpu().numpy().view(np.uint64)
        assert (r.stream_reply[n + 1:] == SENT64).all() and (r.close_off[n:] == SENT64).all()
        r.verdict = cc.verdict_tuples(o.verdict.cpu().numpy().view(np.uint64)[:n].view(PROTO_VERDICT))
        r.stream_first = sf.cpu().numpy().view(np.uint32)[: n + 1]
        r.frames_consumed = self.state.cpu().numpy().view(STREAM_STATE)["consumed"]
        r.proto = None
        setattr(r, self.carries, None)                     # d_state and d_proto stay where they are
        r.spans_left, r.close_left = spans, o.close_off    # ... and so do the spans and the close offsets
        return r

    def final(self):
        st = self.state.cpu().numpy().view(STREAM_STATE)
        pr = self.proto.cpu().numpy().view(PROTO_STATE)
        return [int(x) for x in st[self.carries]], [(int(p["bytes"]), int(p["open"])) for p in pr]


def resident_run(codec, cases, carries, seed, rule, mask, limit, which, keys):
    conns = cases.connections()
    res = Resident(codec, len(conns), sum(len(c.frames) for c in conns) + 1, rule, mask, limit, which, keys, carries)

    def step(*args):
        return res.step(*args)

    step.final = res.final   # d_state and d_proto are read once, behind the last round
    run = kc.drive(step, res.carry, seed, keys, cases=cases, carries=carries)
    return run, res


@functools.lru_cache(maxsize=None)
def model_run(seed):
    limit, validating, rule, mask = VALIDATING[0].values
    keys = sl.send_keys() if mask else None
    return kc.drive(sl.model_step(rule, mask, limit, True), kc.model_carry, seed, keys)


def same_carries(run, model, field):
    """What a connection that was never dropped ends with (a dropped one's
    d_state and d_proto are whatever its last round left)."""
    for j, v in enumerate(model.verdict):
        if v == sl.NONE:
            assert getattr(run, field)[j] == getattr(model, field)[j] and run.proto[j] == model.proto[j], j
    assert run.left == model.left


def check_traffic(run, res, model):
    print("rounds", run.rounds, "bytes read", run.read_bytes, "uploaded", res.uploaded,
          "a loop that uploads every round's wire", res.wire_bytes, "tail bytes carried on the device", res.carried)
    assert res.uploaded == run.read_bytes == model.read_bytes
    assert res.wire_bytes == model.wire_bytes
    assert res.uploaded < res.wire_bytes and res.carried > 0


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", SCHEDULES[:2])
def test_loop(codec, seed):
    """A schedule of cut reads with the wire resident: the checks of the loop
    it replaces, the model driver's run, and the bytes that crossed the bus."""
    limit, validating, rule, mask = VALIDATING[0].values
    keys = sl.send_keys() if mask else None
    run, res = resident_run(codec, sl, "opcode", seed, rule, mask, limit, sl.WHICH, keys)
    sl.check_run(run, limit, validating, rule, mask, "resident, schedule %d" % seed)
    model = model_run(seed)
    assert run.out == model.out and run.verdict == model.verdict
    same_carries(run, model, "opcode")
    assert run.rounds == model.rounds
    check_traffic(run, res, model)


def test_loop_rfc():
    """The first schedule again under WSG_ASSEMBLY_RFC, over the connections
    of tests/rfc_assembly_cases.py (two in five with control frames between
    fragments): d_state[j].ahead is carried on the device beside the bytes."""
    rule, mask = ac.rc.SAME_CLOSE_PONG, 0
    seed = SCHEDULES[0]
    c = ca.Codec(0)
    try:
        c.set_assembly(ac.RFC)
        run, res = resident_run(c, ac, "ahead", seed, rule, mask, 0, ac.WHICH, None)
    finally:
        c.close()
    ac.check_run(run, True, rule, mask, "resident, RFC, schedule %d" % seed)
    model = kc.drive(ac.model_step(rule, mask, True), kc.model_carry, seed, None, cases=ac, carries="ahead")
    assert run.out == model.out and run.verdict == model.verdict
    same_carries(run, model, "ahead")
    check_traffic(run, res, model)


# ------------------------------------------------------------------ the storm
def test_storm(codec):
    """The first 200 connections with their upgrade requests in front.  A round:
    the carry (the connections rejected in the round before dropped through
    d_close_off), wsg_upgrade_streams over the connections not yet
    handshaked, wsg_reply_validated_streams over the handshaked ones, those
    accepted in this round from off + consumed.  The wire stays on the
    device; the span tables of the two calls are cut on the host from the
    carry's, as tests/test_gpu_upgrade_loop.py cuts them."""
    limit, validating, rule, mask = VALIDATING[0].values
    keys = sl.send_keys() if mask else None
    conns = sl.connections()[:N]
    cpu = model_run(0)
    data = [request_of(j) + conns[j].data for j in range(N)]
    frame_cap = sum(len(c.frames) for c in conns) + 1
    res = Resident(codec, N, frame_cap, rule, mask, limit, sl.WHICH, None if keys is None else keys[:N], "opcode")
    rng = np.random.default_rng(2024)
    out = [bytearray() for _ in range(N)]
    pos, shaken, gone, codes = [0] * N, [False] * N, [False] * N, [None] * N
    wire, spans, close_off = None, np.zeros(N, dtype=STREAM_SPAN), None
    rounds = both = 0
    while any(not gone[j] and pos[j] < len(data[j]) for j in range(N)):
        rounds += 1
        assert rounds < 60, "the loop does not end"
        chunks, rd, at = [], np.zeros(N, dtype=STREAM_READ), 0
        for j in range(N):
            new = b""
            if not gone[j]:
                pick = int(rng.integers(0, 10))
                size = pick if pick < 3 else len(data[j]) if pick == 9 else int(rng.integers(3, 400))
                new = data[j][pos[j]: pos[j] + size]
                pos[j] += len(new)
            chunks.append(new)
            rd[j] = (at, len(new))
            at += len(new)
        wire, d_spans = res.carry(wire, spans, close_off, np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), rd)
        table = d_spans.cpu().numpy().view(STREAM_SPAN).copy()   # off and len of every stream; consumed 0
        after = table.copy()                                     # ... as the next carry gets it
        drop = np.full(N, kc.U64_MAX, dtype=np.uint64)
        fresh = [j for j in range(N) if not shaken[j] and not gone[j]]
        if fresh:
            sp = table.copy()
            sp["len"][[j for j in range(N) if j not in set(fresh)]] = 0
            d_sp = dev(sp.view(np.uint8))
            up, resp, resp_off, _ = codec.upgrade_streams(wire, d_sp, max_request=0)
            assert codec.sync_status() == 0
            up = up.cpu().numpy()[: N * 32].view(layout.UPGRADE_DTYPE)
            used = d_sp.cpu().numpy().view(STREAM_SPAN)["consumed"]
            resp, resp_off = resp.cpu().numpy(), resp_off.cpu().numpy()
            for j in fresh:
                out[j] += resp[int(resp_off[j]): int(resp_off[j + 1])].tobytes()
                code = int(up["code"][j])
                if code == layout.UP_INCOMPLETE:
                    continue
                codes[j] = code
                if code == layout.UP_ACCEPTED:   # its frames from off + consumed, in this round
                    shaken[j] = True
                    table["off"][j] += used[j]
                    table["len"][j] -= used[j]
                else:
                    gone[j] = True
                    drop[j] = 0
        serve = [j for j in range(N) if shaken[j] and not gone[j]]
        both += bool(fresh) and bool(serve)
        sp = table.copy()
        sp["len"][[j for j in range(N) if j not in set(serve)]] = 0
        d_sp = dev(sp.view(np.uint8))
        r = res.step(wire, d_sp, None, None, None, None)
        served = d_sp.cpu().numpy().view(STREAM_SPAN)
        for j in serve:
            out[j] += bytes(r.reply[int(r.stream_reply[j]): int(r.stream_reply[j + 1])])
            after[j] = served[j]
            if r.verdict[j] != sl.NONE:   # failed or closed on the device: disconnected
                gone[j] = True
                drop[j] = r.close_off[j]
        spans, close_off = dev(after.view(np.uint8)), dev(drop.view(np.int64))
    assert rounds > 5 and both > 3
    for j in range(N):
        e = layout.upgrade_judge(request_of(j))
        if j in BAD:
            assert codes[j] == BAD[j][1] == e["code"] and e["status"] == 400
            assert bytes(out[j]) == e["resp"], "connection %d sent more than its 400" % j
        else:
            assert codes[j] == layout.UP_ACCEPTED == e["code"], j
            assert bytes(out[j]) == e["resp"] + cpu.out[j], "connection %d (%s)" % (j, conns[j].name)
    total = sum(pos)
    print("rounds", rounds, "uploaded", res.uploaded, "a loop that uploads every round's wire", res.wire_bytes)
    assert res.uploaded == total and res.uploaded < res.wire_bytes
