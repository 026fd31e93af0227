"""A reconnect storm on the GPU: the whole connection life cycle in two calls
a round.

200 connections; each one's bytes are an upgrade request (five of them bad in
different ways) followed by the masked frames of tests/server_loop_cases.py's
connections, delivered in seeded cut reads over rounds.  A round is one
wsg_upgrade_streams over the connections not yet handshaked and one
wsg_reply_validated_streams (tests/test_gpu_validated_loop.py's step) over
the handshaked ones, those accepted in this round included, from off +
consumed.  Everything sent on a connection must be the model's response
followed by what the numpy loop (server_loop_cases.model_step) replies to the
connection's frames; a rejected connection sends its 400 and nothing else."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests import upgrade_cases as uc  # noqa: E402
from tests.test_gpu_upgrade import UpOut  # noqa: E402
from tests.test_gpu_validated_loop import VALIDATING, one_call_step  # noqa: E402

N = 200
BAD = {
    7: (uc.request(uc.four(version=b"Sec-WebSocket-Version: 8")), layout.UP_BAD_VERSION),
    64: (uc.request(uc.four() + [b"no colon"]), layout.UP_BAD_HTTP),
    65: (uc.request(uc.four(upgrade=b"Upgrade: h2c")), layout.UP_BAD_UPGRADE),
    131: (uc.request(uc.four()[:-1]), layout.UP_MISSING),
    199: (uc.request(uc.four(connection=b"Connection: Upgrade, keep-alive")), layout.UP_BAD_CONNECTION),
}
MAX_ROUNDS = 60


def request_of(j):
    """Connection j's upgrade request: the shapes of tests/upgrade_cases.py with a key of its own."""
    if j in BAD:
        return BAD[j][0]
    key = b"Sec-WebSocket-Key: " + uc.key_of_length(24, j)
    if j % 3 == 0:
        return uc.browser_request().replace(b"Sec-WebSocket-Key: x3JJHMbDL1EzLkh9GBhXDw==", key)
    if j % 3 == 1:
        return uc.request(list(uc.RFC_LINES[:3]) + [key] + list(uc.RFC_LINES[4:]))
    return uc.request(uc.four(key=key, connection=b"Connection: keep-alive, Upgrade") + [b"Content-Length: 3"], body=b"abc")


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def test_storm(codec):
    limit, validating, rule, mask = VALIDATING[0].values
    assert validating
    _storm(codec, limit, rule, mask)


def _storm(codec, limit, rule, mask):
    keys = sl.send_keys() if mask else None
    conns = sl.connections()[:N]
    frames_step = one_call_step(codec, rule, mask, limit)
    cpu = sl.drive(sl.model_step(rule, mask, limit, True), 0, keys)   # the numpy loop's replies
    data = [request_of(j) + conns[j].data for j in range(N)]
    rng = np.random.default_rng(2024)
    out = [bytearray() for _ in range(N)]
    pos, pending = [0] * N, [b""] * N
    shaken, opcode, proto = [False] * N, [0] * N, [(0, 0)] * N
    codes = [None] * N
    live = list(range(N))
    rounds = both = 0
    while live:
        assert rounds < MAX_ROUNDS, "the loop does not end"
        rounds += 1
        chunks, spans, at = [], np.zeros(len(live), dtype=layout.STREAM_SPAN), 0
        for s, j in enumerate(live):
            pick = int(rng.integers(0, 10))
            size = pick if pick < 3 else len(data[j]) if pick == 9 else int(rng.integers(3, 400))
            new = data[j][pos[j]: pos[j] + size]
            pos[j] += len(new)
            pending[j] += new
            gap = bytes(int(rng.integers(0, 20)))
            chunks += [gap, pending[j]]
            spans["off"][s], spans["len"][s] = at + len(gap), len(pending[j])
            at += len(gap) + len(pending[j])
        chunks.append(bytes(64))
        wire = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        # the connections not yet handshaked
        fresh = [s for s, j in enumerate(live) if not shaken[j]]
        dead = set()
        if fresh:
            sp = spans[fresh].copy()
            want = layout.upgrade_plan(wire, sp)
            o = UpOut(sp, int(want[3][-1]))
            o.run(codec, torch.from_numpy(wire).cuda())
            assert codec.sync_status() == 0
            o.check(want, sp)
            up = o.up.cpu().numpy()[: len(fresh) * 32].view(layout.UPGRADE_DTYPE)
            used = o.spans.cpu().numpy().view(layout.STREAM_SPAN)["consumed"]
            resp, resp_off = o.resp.cpu().numpy(), o.resp_off.cpu().numpy()
            for k, s in enumerate(fresh):
                j = live[s]
                out[j] += resp[int(resp_off[k]): int(resp_off[k + 1])].tobytes()
                code = int(up["code"][k])
                if code == layout.UP_INCOMPLETE:
                    continue
                codes[j] = code
                if code == layout.UP_ACCEPTED:   # its frames from off + consumed, in this round
                    shaken[j] = True
                    pending[j] = pending[j][int(used[k]):]
                    spans["off"][s] += used[k]
                    spans["len"][s] -= used[k]
                else:
                    dead.add(s)
        # the handshaked ones
        serve = [s for s, j in enumerate(live) if shaken[j]]
        both += bool(fresh) and bool(serve)
        if serve:
            sp = spans[serve].copy()
            frame_cap = int(sp["len"].sum()) // 2 + 1
            r = frames_step(wire, sp, np.array([opcode[live[s]] for s in serve], dtype=np.uint8),
                            [proto[live[s]] for s in serve], None if keys is None else keys[[live[s] for s in serve]],
                            frame_cap)
            for k, s in enumerate(serve):
                j = live[s]
                out[j] += bytes(r.reply[int(r.stream_reply[k]): int(r.stream_reply[k + 1])])
                if r.verdict[k] != sl.NONE:   # failed or closed on the device: disconnected
                    dead.add(s)
                    continue
                pending[j] = pending[j][int(r.bytes_consumed[k]):]
                opcode[j], proto[j] = int(r.opcode[k]), (int(r.proto[k][0]), int(r.proto[k][1]))
        live = [j for s, j in enumerate(live) if s not in dead and pos[j] < len(data[j])]
    assert rounds > 5 and both > 3
    for j in range(N):
        e = layout.upgrade_judge(request_of(j))
        if j in BAD:
            assert codes[j] == BAD[j][1] == e["code"] and e["status"] == 400
            assert bytes(out[j]) == e["resp"], "connection %d sent more than its 400" % j
        else:
            assert codes[j] == layout.UP_ACCEPTED == e["code"], j
            assert bytes(out[j]) == e["resp"] + cpu.out[j], "connection %d (%s)" % (j, conns[j].name)
    assert sum(1 for j in range(N) if j not in BAD and cpu.verdict[j] != sl.NONE) > 20
