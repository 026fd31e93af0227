"""Both ends of the upgrade on the device, each checking the other's bytes.

200 client connections with seeded nonces.  wsg_upgrade_requests builds their
requests; the requests go in seeded cut reads to wsg_upgrade_streams; its
responses, each followed at once by an unmasked greeting text frame from the
oracle, go in seeded cut reads to wsg_upgrade_client_streams, one call a round
over the streams not yet decided.  Eight connections' responses are tampered
with in transit.  Every untampered client must be accepted with consumed 148
and wsg_decode_streams over its bytes from there on must deliver its greeting;
every tampered one gets the model's code."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
import oracle  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests.test_gpu_frames import dev  # noqa: E402
from tests.test_gpu_upgrade import UpOut  # noqa: E402
from tests.test_gpu_upgrade_client import UcOut, padded_dev  # noqa: E402

N = 200
MAX_ROUNDS = 60
HEAD = (b"GET /chat HTTP/1.1\r\nHost: localhost\r\nOrigin: http://localhost\r\nUpgrade: websocket\r\n"
        b"Connection: Upgrade\r\nSec-WebSocket-Key: ")
TEMPLATE = HEAD + b"=" * 24 + b"\r\nSec-WebSocket-Protocol: chat, superchat\r\nSec-WebSocket-Version: 13\r\nContent-Length: 0\r\n\r\n"


def tamper(j, resp):
    """What happens to connection j's 148 response bytes in transit (None: nothing)."""
    at = resp.find(b"Accept: ") + 8
    if j in (3, 150):       # an accept letter changed
        k = at + (5 if j == 3 else 25)
        return resp[:k] + (b"A" if resp[k:k + 1] != b"A" else b"B") + resp[k + 1:], layout.UC_BAD_ACCEPT
    if j in (17, 64):       # Upgrade changed
        return resp.replace(b"Upgrade: websocket", b"Upgrade: websockex"), layout.UC_BAD_UPGRADE
    if j in (65, 199):      # another status
        return resp.replace(b" 101 Switching Protocols", b" 200 OK"), layout.UC_NOT_101
    if j == 100:            # a header line without ':'
        return resp.replace(b"Connection: Upgrade", b"Connection  Upgrade"), layout.UC_BAD_HTTP
    if j == 128:            # never completed
        return resp[:120], layout.UC_INCOMPLETE
    return None


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def cut_rounds(rng, data, step):
    """Deliver data[j] in seeded cut reads, one wire a round over the
    connections ``step`` has not decided: step(wire, spans, live) returns the
    positions (in live) that are decided."""
    n = len(data)
    pos, pending = [0] * n, [b""] * n
    live = list(range(n))
    rounds = 0
    while live:
        assert rounds < MAX_ROUNDS, "the loop does not end"
        rounds += 1
        chunks, spans, at = [], np.zeros(len(live), dtype=layout.STREAM_SPAN), 0
        for s, j in enumerate(live):
            pick = int(rng.integers(0, 10))
            size = pick if pick < 3 else len(data[j]) if pick == 9 else int(rng.integers(3, 120))
            new = data[j][pos[j]: pos[j] + size]
            pos[j] += len(new)
            pending[j] += new
            gap = bytes(int(rng.integers(0, 20)))
            chunks += [gap, pending[j]]
            spans["off"][s], spans["len"][s] = at + len(gap), len(pending[j])
            at += len(gap) + len(pending[j])
        wire = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        decided = step(wire, spans, live)
        live = [j for s, j in enumerate(live) if s not in decided and pos[j] < len(data[j])]
    return rounds


def test_both_ends(codec):
    rng = np.random.default_rng(6455)
    nonces = rng.integers(0, 256, 16 * N, dtype=np.uint8)
    nonce = [nonces[16 * j:16 * j + 16].tobytes() for j in range(N)]
    # the requests, on the device
    req = codec.upgrade_requests(padded_dev(np.frombuffer(TEMPLATE, dtype=np.uint8)), len(HEAD), dev(nonces))
    assert codec.sync_status() == 0
    req = req.cpu().numpy()[: N * len(TEMPLATE)].reshape(N, len(TEMPLATE))
    requests = [req[j].tobytes() for j in range(N)]
    for j in range(N):
        assert requests[j] == layout.upgrade_request(TEMPLATE, len(HEAD), nonce[j])

    # the server's half
    responses = [b""] * N

    def serve(wire, spans, live):
        want = layout.upgrade_plan(wire, spans)
        o = UpOut(spans, int(want[3][-1]))
        o.run(codec, padded_dev(wire))
        assert codec.sync_status() == 0
        o.check(want, spans)
        up = o.up.cpu().numpy()[: len(live) * 32].view(layout.UPGRADE_DTYPE)
        resp, resp_off = o.resp.cpu().numpy(), o.resp_off.cpu().numpy()
        decided = set()
        for s, j in enumerate(live):
            if int(up["code"][s]) != layout.UP_INCOMPLETE:
                assert int(up["code"][s]) == layout.UP_ACCEPTED, j
                responses[j] = resp[int(resp_off[s]): int(resp_off[s + 1])].tobytes()
                decided.add(s)
        return decided

    assert cut_rounds(rng, requests, serve) > 3
    assert all(len(r) == 148 for r in responses)

    # the greetings: unmasked text frames from the oracle
    texts = [b"hello, client %d" % j + b"!" * (j % 7) for j in range(N)]
    desc = np.zeros(N, dtype=layout.SEND_DESC)
    desc["len"] = [len(t) for t in texts]
    desc["src_off"][1:] = np.cumsum(desc["len"][:-1])
    desc["opcode"] = layout.WS_FIN | layout.WS_TEXT
    gw, goff = oracle.encode_batch(np.frombuffer(b"".join(texts), dtype=np.uint8), desc)
    greeting = [gw[int(goff[j]): int(goff[j + 1])].tobytes() for j in range(N)]
    assert greeting[0] == bytes([0x81, len(texts[0])]) + texts[0]

    # the wire to the clients, eight of them tampered with
    changed = {j: tamper(j, responses[j]) for j in range(N) if tamper(j, responses[j])}
    assert len(changed) == 8
    to_client = [(changed[j][0] if j in changed else responses[j]) + (greeting[j] if j != 128 else b"") for j in range(N)]
    expect = [layout.upgrade_client_judge(to_client[j], nonce[j]) for j in range(N)]
    for j, (_, code) in changed.items():
        assert expect[j]["code"] == code, j

    # the client's half
    codes, consumed, totals = [None] * N, [0] * N, np.zeros(3, dtype=np.uint64)

    def judge(wire, spans, live):
        nn = np.concatenate([nonces[16 * j:16 * j + 16] for j in live])
        want = layout.upgrade_client_plan(wire, spans, nn)
        o = UcOut(spans, nn)
        o.run(codec, padded_dev(wire))
        assert codec.sync_status() == 0
        o.check(want, spans)
        up = o.up.cpu().numpy()[: len(live) * 32].view(layout.UPGRADE_REPLY_DTYPE)
        used = o.spans.cpu().numpy().view(layout.STREAM_SPAN)["consumed"]
        cnt = o.count.cpu().numpy().view(np.uint64)[:3]
        totals[:2] += cnt[:2]
        decided = set()
        for s, j in enumerate(live):
            if int(up["code"][s]) != layout.UC_INCOMPLETE:
                codes[j], consumed[j] = int(up["code"][s]), int(used[s])
                decided.add(s)
        return decided

    assert cut_rounds(rng, to_client, judge) > 3
    for j in range(N):
        if j in changed:
            want = changed[j][1]
            assert codes[j] == (None if want == layout.UC_INCOMPLETE else want), j
        else:
            assert (codes[j], consumed[j]) == (layout.UC_ACCEPTED, 148), j
    assert [int(x) for x in totals[:2]] == [N - 8, 7]

    # the accepted connections' bytes from consumed on: their greetings
    accepted = [j for j in range(N) if codes[j] == layout.UC_ACCEPTED]
    parts, spans, at = [], np.zeros(len(accepted), dtype=layout.STREAM_SPAN), 0
    for s, j in enumerate(accepted):
        rest = to_client[j][consumed[j]:]
        spans["off"][s], spans["len"][s] = at, len(rest)
        parts.append(rest)
        at += len(rest)
    wire = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    d_spans = dev(spans.view(np.uint8))
    msg, msgs, count, _, _, _, _, n_frames = codec.decode_streams(padded_dev(wire), d_spans, frame_cap=len(accepted) + 8)
    assert codec.sync_status() == 0
    assert n_frames == len(accepted) and int(count.cpu()[0]) == len(accepted)
    recs = msgs.cpu().numpy()[: len(accepted) * layout.MSG.itemsize].view(layout.MSG)
    got = msg.cpu().numpy()
    for s, j in enumerate(accepted):
        assert int(recs["stream"][s]) == s and int(recs["opcode"][s]) & 0x0F == layout.WS_TEXT
        assert got[int(recs["off"][s]): int(recs["off"][s]) + int(recs["len"][s])].tobytes() == texts[j], j
    used = d_spans.cpu().numpy().view(layout.STREAM_SPAN)["consumed"]
    assert [int(u) for u in used] == [len(greeting[j]) for j in accepted]
