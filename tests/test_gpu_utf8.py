"""wsg_check_utf8 on the GPU: text messages and close reasons validated where
wsg_decode_messages left them.

Every call goes through run(): the batch is decoded on the device and checked
with no synchronisation between the two calls; d_valid and d_result start as
the 0xA5 sentinel; afterwards every d_valid[m], m < M, and all four d_result
words are compared, and d_valid[M:] must still hold the sentinel.  The
expected values come from Python's bytes.decode("utf-8") alone (len, or
e.start; tests/utf8_cases.py:want), applied to the data that
layout.message_plan and the oracle give for each message."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_STATE  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import utf8_cases as uc  # noqa: E402

SENTINEL = 0xA5
SENTINEL64 = int(np.frombuffer(bytes([SENTINEL]) * 8, dtype=np.int64)[0])
U64_MAX = 2 ** 64 - 1
TEXT, BINARY, CLOSE, PING = 0x81, 0x82, 0x88, 0x89
DEFAULT = ca.UTF8_TEXT | ca.UTF8_CLOSE


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def model(batch):
    """(msgs, count, dense bytes) of the batch: layout.message_plan over the oracle's decode."""
    out, info = batch.oracle_decode()
    msgs, count, state = layout.message_plan(info, batch.stream_first, None, payload=out)
    return msgs, count, mc.dense(out, info, batch.stream_first, state)


def selected(m, which):
    kind, opcode = int(m["kind"]), int(m["opcode"])
    return bool(which & ca.UTF8_EVERY) or bool(which & ca.UTF8_TEXT and kind == ca.CB_RECEIVED and opcode == 1) or \
        bool(which & ca.UTF8_CLOSE and kind == ca.CB_CLOSE)


def expected(msgs, buf, which, bound, room):
    """(valid[M], result) from Python's decoder."""
    M = min(len(msgs), room)
    valid, bad, checked, nbytes = [], [], 0, 0
    for m in range(M):
        off, size = int(msgs["off"][m]), int(msgs["len"][m])
        v = size
        if selected(msgs[m], which) and off + size <= bound:
            checked += 1
            nbytes += size
            v = uc.want(bytes(buf[off: off + size]))
            if v < size:
                bad.append(m)
        valid.append(v)
    return valid, [len(bad), bad[0] if bad else U64_MAX, checked, nbytes]


def _on(stream):
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def outputs(msg_room):
    """d_valid (3 words past msg_room) and d_result, holding the sentinel."""
    return (torch.full((max(msg_room, 1) + 3,), SENTINEL64, dtype=torch.int64, device="cuda"),
            torch.full((4,), SENTINEL64, dtype=torch.int64, device="cuda"))


def decode(codec, batch, msg_cap=None, stream=None):
    """wsg_decode_messages of the batch, not synchronised.  Returns (d_msg, d_msgs, d_count)."""
    n = batch.n
    cap = len(batch.wire) if msg_cap is None else msg_cap
    d_msg = torch.full((max(cap, 16) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msgs = torch.full((max(n, 1) * MSG.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    wire = dev(batch.wire) if len(batch.wire) else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    fs, sf = dev(batch.fs.view(np.int64)), dev(batch.stream_first)
    if stream is not None:
        torch.cuda.synchronize()   # the buffers are ready before the side stream starts
    with _on(stream):
        codec.decode_messages(wire, fs, sf, msg=d_msg, msg_cap=cap, msgs=d_msgs, count=d_count)
    return d_msg, d_msgs, d_count


def check(codec, d_msg, d_msgs, d_count, which, msg_cap, msg_room, want_valid, want_result, stream=None, outs=None):
    """wsg_check_utf8 on sentinel outputs and the comparison of everything it writes."""
    d_valid, d_result = outs if outs is not None else outputs(msg_room)
    with _on(stream):
        codec.check_utf8(d_msg, d_msgs, d_count, which=which, msg_cap=msg_cap, msg_room=msg_room, valid=d_valid,
                         result=d_result)
    if stream is not None:
        stream.synchronize()
    valid = d_valid.cpu().numpy().view(np.uint64)
    result = [int(x) for x in d_result.cpu().numpy().view(np.uint64)]
    M = len(want_valid)
    got = [int(x) for x in valid[:M]]
    assert got == want_valid, [(m, g, w) for m, (g, w) in enumerate(zip(got, want_valid)) if g != w][:10]
    assert (valid[M:].view(np.int64) == SENTINEL64).all()   # entries at M and beyond are not written
    assert result == want_result
    return got, result


def run(codec, batch, which=DEFAULT, msg_cap=None, msg_room=None, ref=None, stream=None):
    """Decode + check on one stream, no synchronisation between; every
    output against the decoder.  Returns (msgs, valid, result)."""
    msgs, count, buf = ref if ref is not None else model(batch)
    cap = len(batch.wire) if msg_cap is None else msg_cap
    room = max(batch.n, 1) if msg_room is None else msg_room
    want_valid, want_result = expected(msgs, buf, which, min(cap, int(count[1])), room)
    outs = outputs(room)                                     # made first: nothing between the two calls
    d_msg, d_msgs, d_count = decode(codec, batch, stream=stream)
    valid, result = check(codec, d_msg, d_msgs, d_count, which, cap, room, want_valid, want_result, stream=stream,
                          outs=outs)
    assert codec.sync_status() == 0
    got = d_msgs.cpu().numpy().view(MSG)[: len(msgs)]
    mc.same_fields(got, msgs, mc.MSG_FIELDS)                 # the table the expected values were made for
    assert [int(x) for x in d_count.cpu().numpy()] == [int(x) for x in count]
    if len(buf) <= 1 << 16:   # the numpy restatement agrees with the decoder too (a Python loop over the bytes)
        pv, pr = layout.utf8_plan(msgs[:room], buf, which, msg_cap=cap)
        assert [int(x) for x in pv] == want_valid and [int(x) for x in pr] == want_result
    return msgs, valid, result


def frame(b0, data, key=None):
    return mc.raw_frame(b0, data, key=key)


# ------------------------------------------------------------------ 1. KAT
def test_kat_text_then_binary(codec):
    k = uc.kat()
    names = sorted(k)
    text = mc.Batch([[frame(TEXT, k[nm], key=7 + i) for i, nm in enumerate(names)]])
    msgs, valid, result = run(codec, text, ca.UTF8_TEXT)
    assert valid == [uc.want(k[nm]) for nm in names] and result[2] == len(names)
    at = {nm: valid[i] for i, nm in enumerate(names)}
    for nm in ("empty", "ascii", "first_1", "last_1", "first_2", "last_2", "first_3", "last_3", "first_4", "last_4",
               "mixed"):
        assert at[nm] == len(k[nm]), nm
    for nm in ("overlong_2a", "overlong_2b", "overlong_3", "overlong_4", "surrogate_lo", "surrogate_hi",
               "above_10ffff", "f5", "ff", "stray_80", "lead2_ascii", "lead3_ascii", "lead4_ascii", "trunc_c2_1",
               "trunc_euro_1", "trunc_euro_2", "trunc_grin_1", "trunc_grin_2", "trunc_grin_3"):
        assert at[nm] == 0, nm
    assert at["stray_after_text"] == 3 and at["lead3_ascii_3rd"] == 0 and at["text_trunc_euro_2"] == 8
    run(codec, text, ca.UTF8_EVERY)
    run(codec, text, DEFAULT)
    binary = mc.Batch([[frame(BINARY, k[nm], key=7 + i) for i, nm in enumerate(names)]])
    _, valid, result = run(codec, binary, ca.UTF8_TEXT)
    assert valid == [len(k[nm]) for nm in names] and result == [0, U64_MAX, 0, 0]      # nothing is checked
    _, valid, result = run(codec, binary, ca.UTF8_EVERY)
    assert valid == [uc.want(k[nm]) for nm in names] and result[2] == len(names)       # everything is


# ------------------------------------------------------- 2. position sweep
def test_position_sweep(codec):
    """A 64-byte ASCII message with F0 9F 98 80 at every offset 0..60, the
    same with its third byte 41, and the sequence cut by the message's end;
    a binary message of 0..15 bytes in front of each gives the message's
    start every alignment to the 16-byte chunk."""
    base = bytes(range(0x30, 0x70))
    cases = []
    for at in range(61):
        cases.append((base[:at] + uc.GRIN + base[at + 4:], 64))
        cases.append((base[:at] + b"\xf0\x9f\x41\x80" + base[at + 4:], at))
    for cut in (1, 2, 3):
        cases.append((base[: 64 - cut] + uc.GRIN[:cut], 64 - cut))
    frames, used, aligns = [], 0, {}
    for ci, (text, _) in enumerate(cases):
        for a in range(16):
            pad = (a - used) % 16
            frames += [frame(BINARY, b"\xff" * pad, key=3), frame(TEXT, text, key=0x01020304 + ci)]
            aligns.setdefault(ci, set()).add((used + pad) % 16)
            used += pad + 64
    assert all(len(s) == 16 for s in aligns.values())
    msgs, valid, result = run(codec, mc.Batch([frames]))
    assert valid[1::2] == [w for _, w in cases for _ in range(16)]
    assert {int(o) % 16 for o in msgs["off"][1::2]} == set(range(16))
    assert result[2] == len(cases) * 16 and result[3] == 64 * len(cases) * 16


# -------------------------------------- 3. no context across a boundary
def test_no_context_across_message_boundary(codec):
    a, b = b"price: \xe2\x82", b"\xac and more"
    for fill in range(0, 20, 3):     # the boundary at several places of a chunk
        head = frame(BINARY, bytes(fill))
        _, valid, _ = run(codec, mc.Batch([[head, frame(TEXT, a, key=1), frame(TEXT, b, key=2)]]))
        assert valid == [fill, len(a) - 2, 0]
        _, valid, _ = run(codec, mc.Batch([[head, frame(TEXT, a, key=1)], [frame(TEXT, b, key=2)]]))
        assert valid == [fill, len(a) - 2, 0]
        _, valid, result = run(codec, mc.Batch([[head, frame(BINARY, a, key=1), frame(TEXT, b, key=2)]]))
        assert valid == [fill, len(a), 0] and result == [1, 2, 1, len(b)]


# ------------------------------------------------------------ 4. fragments
def _fragments(data, cuts, keys):
    """data cut at `cuts` into len(cuts) + 1 frames: TEXT, continuations, the last with FIN."""
    edges = [0] + list(cuts) + [len(data)]
    parts = [data[edges[i]: edges[i + 1]] for i in range(len(edges) - 1)]
    ops = [0x01] + [0x00] * (len(parts) - 1)
    ops[-1] |= 0x80
    return [frame(op, p, key=k) for op, p, k in zip(ops, parts, keys)]


@pytest.mark.parametrize("masked", [True, False])
def test_sequences_split_over_fragments(codec, masked):
    streams, want_valid = [], []
    for seq in (uc.EURO, uc.GRIN):
        for nfrag in (2, 3, 4):
            data = b"ab" + seq + b"cd"
            inner = list(range(3, 2 + len(seq)))                 # the cuts inside the sequence
            cuts = (inner + [inner[-1]] * 4)[: nfrag - 1]          # (an empty fragment where they run out)
            keys = [0x11111111 * (i + 1) + nfrag if masked else None for i in range(nfrag)]
            streams.append(_fragments(data, cuts, keys))
            want_valid.append(len(data))
            bad = bytearray(data)
            bad[cuts[0]] = 0x41                                    # the byte that begins the second fragment
            streams.append(_fragments(bytes(bad), cuts, keys))
            want_valid.append(2)                                   # the sequence's start in the assembled message
    # a tail (frames after the stream's last FIN frame) with invalid bytes: in no message
    streams.append([frame(TEXT, b"fine", key=5 if masked else None), frame(0x01, b"\xff\xfe\x80")])
    want_valid.append(4)
    msgs, valid, result = run(codec, mc.Batch(streams))
    assert valid == want_valid and result[0] == 6 and result[1] == 1
    assert list(msgs["nframes"]) == [2, 2, 3, 3, 4, 4] * 2 + [1]


# -------------------------------------------------------- 5. close reasons
def test_close_reasons(codec):
    bodies = [b"\x03\xe8", b"", b"\x03\xe8bye \xe2\x82\xac", b"\x03\xe8by\xffe", b"\x03", b"\x80",
              b"\x03\xe9" + uc.GRIN[:2]]
    batch = mc.Batch([[frame(CLOSE, b, key=9 + i)] for i, b in enumerate(bodies)])
    msgs, valid, result = run(codec, batch, ca.UTF8_CLOSE)
    assert list(msgs["len"]) == [0, 0, 7, 4, 1, 1, 2]
    assert valid == [0, 0, 7, 2, 1, 0, 0]               # counted from off, past the status
    assert result == [3, 3, 7, 15]
    _, valid, result = run(codec, batch, ca.UTF8_TEXT)  # not checked
    assert valid == [0, 0, 7, 4, 1, 1, 2] and result == [0, U64_MAX, 0, 0]
    _, valid, result = run(codec, batch, 0)
    assert valid == [0, 0, 7, 4, 1, 1, 2] and result == [0, U64_MAX, 0, 0]
    run(codec, batch, DEFAULT)


# --------------------------------------------------- 6. many small messages
def test_many_small_messages(codec):
    rng = np.random.default_rng(66)
    streams = [[] for _ in range(37)]
    run_at, total = 2100, 5000
    i = 0
    while i < total:
        j = int(rng.integers(0, 37))
        if i == run_at:   # 300 consecutive empty text messages, then an invalid one, in one stream
            streams[j] += [frame(TEXT, b"", key=int(rng.integers(1, 2 ** 32))) for _ in range(300)]
            streams[j].append(frame(TEXT, b"\xe2\x82", key=77))
            i += 301
            continue
        text = uc.mixed_text(rng, int(rng.integers(0, 41)))
        if text and rng.random() < 0.25:
            text = uc.corrupt(rng, text)
        b0 = int(rng.choice([TEXT, TEXT, BINARY, PING, CLOSE]))
        streams[j].append(frame(b0, text, key=int(rng.integers(0, 2 ** 32)) if rng.random() < 0.7 else None))
        i += 1
    batch = mc.Batch(streams)
    ref = model(batch)
    msgs, valid, result = run(codec, batch, DEFAULT, ref=ref)
    assert len(msgs) == 5000 and result[0] > 400 and result[2] > 2500
    empties = np.flatnonzero((msgs["len"] == 0) & (msgs["opcode"] == 1))
    assert len(empties) >= 300
    run(codec, batch, ca.UTF8_EVERY, ref=ref)
    run(codec, batch, ca.UTF8_TEXT, ref=ref)


# ------------------------------------- 7. one large message, later passes
def test_large_message_later_passes():
    os.environ["WSG_UTF8_BLOCKS_PER_CU"] = "1"
    try:
        c = ca.Codec(0)
    finally:
        del os.environ["WSG_UTF8_BLOCKS_PER_CU"]
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        per_pass = cus * 4096                      # one block per CU, 256 chunks of 16 bytes per block and pass
        n = 3 * per_pass + 5
        assert -(-n // 4096) > cus and n > 2 * per_pass    # the grid is capped at cus blocks; a third pass is reached
        rng = np.random.default_rng(7)
        spots = [0, 15, 16, 17, per_pass - 1, per_pass, n - 1]
        edges = sorted(set(spots + [s + 1 for s in spots] + [n]))
        text = bytearray()
        for lo, hi in zip([0] + edges, edges):     # a code point begins at every spot and behind it
            text += uc.mixed_text(rng, hi - lo)
        assert len(text) == n and uc.want(text) == n
        key = 0xC3A5F00D
        batch = mc.Batch([[frame(TEXT, bytes(text), key=key)]])
        msgs, count, buf = model(batch)
        assert int(msgs["len"][0]) == n
        _, valid, result = run(c, batch, ca.UTF8_TEXT, ref=(msgs, count, buf))
        assert valid == [n] and result == [0, U64_MAX, 1, n]
        for s in spots:
            bad = bytearray(text)
            bad[s] = 0xFF
            buf2 = buf.copy()
            buf2[s] = 0xFF
            _, valid, result = run(c, mc.Batch([[frame(TEXT, bytes(bad), key=key)]]), ca.UTF8_TEXT,
                                   ref=(msgs, count, buf2))
            assert valid == [s] and result == [1, 0, 1, n], s
    finally:
        c.close()


# ------------------------------------------------------------- 8. bounds
def _mixed_batch(seed, n=40):
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        text = uc.mixed_text(rng, int(rng.integers(1, 60)))
        if i % 3 == 1:
            text = uc.corrupt(rng, text)
        frames.append(frame(TEXT if i % 5 else BINARY, text, key=100 + i))
    return mc.Batch([frames[: n // 2], frames[n // 2:]])


def test_msg_cap_below_bytes_used(codec):
    batch = _mixed_batch(81)
    msgs, count, buf = model(batch)
    cut = len(msgs) // 2
    cap = int(msgs["off"][cut]) + int(msgs["len"][cut]) - 1      # message `cut` ends one byte past it
    assert cap < int(count[1])
    d_msg, d_msgs, d_count = decode(codec, batch)
    torch.cuda.synchronize()
    d_msg[cap:] = 0xFF                                           # never read as data
    buf_ff = buf.copy()
    buf_ff[cap:] = 0xFF
    for which in (ca.UTF8_EVERY, DEFAULT):
        want_valid, want_result = expected(msgs, buf, which, cap, batch.n)
        assert want_valid[cut:] == [int(x) for x in msgs["len"][cut:]]
        assert want_result[2] == sum(selected(m, which) for m in msgs[:cut])
        check(codec, d_msg, d_msgs, d_count, which, cap, batch.n, want_valid, want_result)
    # ... and the whole buffer with those bytes FF reads them: the bound is what kept them out
    want_valid, want_result = expected(msgs, buf_ff, ca.UTF8_EVERY, len(buf), batch.n)
    assert want_valid[cut] < int(msgs["len"][cut])
    check(codec, d_msg, d_msgs, d_count, ca.UTF8_EVERY, len(batch.wire), batch.n, want_valid, want_result)
    # a cap that is no multiple of 16 and cuts a message's chunk: msg_cap 0 and 1 too
    for cap in (0, 1, int(msgs["off"][3]) + 1, int(msgs["off"][5]) + int(msgs["len"][5])):
        want_valid, want_result = expected(msgs, buf_ff, ca.UTF8_EVERY, cap, batch.n)
        check(codec, d_msg, d_msgs, d_count, ca.UTF8_EVERY, cap, batch.n, want_valid, want_result)


def test_msg_room_below_count_and_no_messages(codec):
    batch = _mixed_batch(82)
    ref = model(batch)
    for room in (0, 1, 7, batch.n - 1):
        _, valid, _ = run(codec, batch, ca.UTF8_EVERY, msg_room=room, ref=ref)
        assert len(valid) == room
    # no message: a tail only, and no frame at all
    for empty in (mc.Batch([[frame(0x01, b"\xff tail")]]), mc.Batch([[]]), mc.Batch([])):
        _, valid, result = run(codec, empty, ca.UTF8_EVERY)
        assert valid == [] and result == [0, U64_MAX, 0, 0]


def test_after_a_decode_without_room(codec):
    """The decode latches WSG_ENOMEM and writes no byte of d_msg (it stays the
    sentinel, which is no UTF-8); d_count[1] holds the size needed.  No
    message fits below msg_cap: nothing is checked, nothing is read."""
    rng = np.random.default_rng(83)
    batch = mc.Batch([[frame(TEXT, uc.mixed_text(rng, 700 + i), key=5 + i) for i in range(6)]])
    msgs, count, buf = model(batch)
    cap = 512
    d_msg, d_msgs, d_count = decode(codec, batch, msg_cap=cap)
    want_valid = [int(x) for x in msgs["len"]]
    check(codec, d_msg, d_msgs, d_count, ca.UTF8_EVERY, cap, batch.n, want_valid, [0, U64_MAX, 0, 0])
    assert codec.sync_status() == ca.WSG_ENOMEM
    assert (d_msg.cpu().numpy() == SENTINEL).all()
    assert [int(x) for x in d_count.cpu().numpy()] == [6, int(count[1])]
    assert codec.sync_status() == 0


# ---------------------------------------------------------- 9. arguments
def test_null_and_misaligned_operands(codec):
    batch = _mixed_batch(91, 8)
    d_msg, d_msgs, d_count = decode(codec, batch)
    d_valid = torch.full((8,), SENTINEL64, dtype=torch.int64, device="cuda")
    d_result = torch.full((4,), SENTINEL64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    good = [d_msg.data_ptr(), len(batch.wire), d_msgs.data_ptr(), d_count.data_ptr(), 8, ca.UTF8_EVERY,
            d_valid.data_ptr(), d_result.data_ptr()]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return codec._L.wsg_check_utf8(codec._ctx, vp(a[0]), a[1], vp(a[2]), vp(a[3]), a[4], a[5], vp(a[6]), vp(a[7]),
                                       None)

    assert codec._L.wsg_check_utf8(None, vp(good[0]), good[1], vp(good[2]), vp(good[3]), 8, 4, vp(good[6]),
                                   vp(good[7]), None) == ca.WSG_EINVAL
    for change in (dict(a0=None), dict(a2=None), dict(a3=None), dict(a6=None), dict(a7=None),
                   dict(a0=good[0] + 8), dict(a0=good[0] + 1), dict(a2=good[2] + 4), dict(a3=good[3] + 4),
                   dict(a6=good[6] + 2), dict(a7=good[7] + 1)):
        assert call(**change) == ca.WSG_EINVAL, change
    torch.cuda.synchronize()
    assert (d_valid.cpu().numpy() == SENTINEL64).all() and (d_result.cpu().numpy() == SENTINEL64).all()
    # NULL buffers are fine where nothing can be read or written through them
    assert call(a0=None, a1=0) == 0 and call(a2=None, a6=None, a4=0) == 0
    assert call() == 0
    assert codec.sync_status() == 0
    assert [int(x) for x in d_result.cpu().numpy().view(np.uint64)][2] == batch.n


def test_checked_launch_refuses_short_valid_block():
    """$WSG_CHECK=1 (read at wsg_create): a d_valid block one word short is
    WSG_EINVAL and nothing is launched; a block of msg_room words runs.  The
    blocks are exact device allocations (torch's allocator hands out views of
    larger segments)."""
    os.environ["WSG_CHECK"] = "1"
    try:
        c = ca.Codec(0)
    finally:
        del os.environ["WSG_CHECK"]
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    vp = ctypes.c_void_p
    room = (2 << 20) // 8 + 1                # room words end 8 bytes past 2 MiB, room - 1 end at it
    blocks = []

    def hip_block(nbytes):
        p = vp()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        assert hip.hipMemset(p, SENTINEL, ctypes.c_size_t(nbytes)) == 0
        blocks.append(p)
        return p.value

    def read_block(ptr, nbytes):
        host = np.empty(nbytes, dtype=np.uint8)
        assert hip.hipMemcpy(vp(host.ctypes.data), vp(ptr), ctypes.c_size_t(nbytes), 2) == 0   # device to host
        return host

    try:
        batch = mc.Batch([[frame(TEXT, b"ok", key=1), frame(TEXT, b"\xc3", key=2), frame(TEXT, uc.EURO, key=3)]])
        d_msg, d_msgs, d_count = decode(c, batch)
        d_table = torch.zeros(room * MSG.itemsize, dtype=torch.uint8, device="cuda")
        d_table[: d_msgs.numel()] = d_msgs
        d_result = torch.full((4,), SENTINEL64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def call(valid_ptr):
            rc = c._L.wsg_check_utf8(c._ctx, vp(d_msg.data_ptr()), len(batch.wire), vp(d_table.data_ptr()),
                                     vp(d_count.data_ptr()), room, ca.UTF8_TEXT, vp(valid_ptr),
                                     vp(d_result.data_ptr()), None)
            torch.cuda.synchronize()
            return rc

        short = hip_block((room - 1) * 8)
        assert call(short) == ca.WSG_EINVAL
        assert (read_block(short, (room - 1) * 8) == SENTINEL).all()
        assert (d_result.cpu().numpy() == SENTINEL64).all()
        full = hip_block(room * 8)
        assert call(full) == 0
        got = read_block(full, room * 8).view(np.uint64)
        assert [int(x) for x in got[:3]] == [2, 0, 3] and (got[3:].view(np.int64) == SENTINEL64).all()
        assert [int(x) for x in d_result.cpu().numpy().view(np.uint64)] == [1, 1, 3, 6]
        assert c.sync_status() == 0
    finally:
        c.close()
        for p in blocks:
            hip.hipFree(p)


# -------------------------------------------------------------- 10. async
def test_side_stream_no_synchronisation(codec):
    batch = _mixed_batch(101, 200)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _, valid, result = run(codec, batch, DEFAULT, stream=st)
    assert result[0] > 0


def test_graph_replay_follows_new_bytes():
    """decode_messages + check_utf8 captured into one graph (after one plain
    run, so that the decode's scratch has grown; the check has none) and
    replayed on a wire whose bytes were changed in place."""
    c = ca.Codec(0)   # a context of its own: the graph names its scratch
    try:
        rng = np.random.default_rng(102)
        sizes = [int(rng.integers(1, 200)) for _ in range(64)]
        texts = [uc.mixed_text(rng, s) for s in sizes]

        def batch_of(texts):
            frames = [frame(TEXT if i % 4 else BINARY, t) for i, t in enumerate(texts)]   # unmasked: same layout
            return mc.Batch([frames[:30], frames[30:]])

        first = batch_of(texts)
        n, cap = first.n, len(first.wire)
        d_wire = dev(first.wire)
        fs, sf = dev(first.fs.view(np.int64)), dev(first.stream_first)
        d_msg = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
        d_msgs = torch.empty(n * MSG.itemsize, dtype=torch.uint8, device="cuda")
        d_count = torch.empty(2, dtype=torch.int64, device="cuda")
        d_state = torch.zeros(2 * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
        d_info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
        d_valid = torch.empty(n, dtype=torch.int64, device="cuda")
        d_result = torch.empty(4, dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()

        def calls():
            c.decode_messages(d_wire, fs, sf, state=d_state, msg=d_msg, msg_cap=cap, msgs=d_msgs, count=d_count,
                              info=d_info)
            c.check_utf8(d_msg, d_msgs, d_count, which=ca.UTF8_TEXT, msg_cap=cap, msg_room=n, valid=d_valid,
                         result=d_result)

        def verify(batch):
            assert c.sync_status(st) == 0
            msgs, count, buf = model(batch)
            want_valid, want_result = expected(msgs, buf, ca.UTF8_TEXT, int(count[1]), n)
            assert [int(x) for x in d_valid.cpu().numpy().view(np.uint64)] == want_valid
            assert [int(x) for x in d_result.cpu().numpy().view(np.uint64)] == want_result
            return want_result

        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            calls()
        assert verify(first) == [0, U64_MAX, sum(1 for i in range(n) if i % 4), sum(s for i, s in enumerate(sizes) if i % 4)]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            calls()
        for replay in range(3):
            changed = [uc.corrupt(rng, t) if rng.random() < 0.4 else uc.mixed_text(rng, len(t)) for t in texts]
            batch = batch_of(changed)
            assert len(batch.wire) == cap and np.array_equal(batch.fs, first.fs)
            d_wire.copy_(dev(batch.wire))
            d_valid.fill_(SENTINEL64)
            d_result.fill_(SENTINEL64)
            d_state.zero_()
            torch.cuda.synchronize()
            g.replay()
            assert verify(batch)[0] > 0
    finally:
        c.close()


# ------------------------------------------------- 11. the 1 KiB wave edges
# A wave of k_utf8_scan owns 1 KiB of d_msg, a 16-byte chunk per lane; the 4
# bytes on either side of a chunk come from the neighbouring lanes' registers,
# except lane 0's `pre` and lane 63's `post`, which those lanes load themselves
# (the `post` byte by byte where the bound cuts it).  Only a multi-byte
# sequence on a wave edge, or a bound 1 to 3 bytes behind one, lets those
# loads decide a verdict.
EDGE_BASE = bytes(range(0x30, 0x60))   # 48 ASCII bytes
EDGE_AT = 20                           # the sequence's offset in its message


def _edge_codec(one_block):
    if not one_block:
        return ca.Codec(0)
    os.environ["WSG_UTF8_BLOCKS_PER_CU"] = "1"
    try:
        return ca.Codec(0)
    finally:
        del os.environ["WSG_UTF8_BLOCKS_PER_CU"]


def _edge_waves(one_block):
    """The edges 1024 w looked at; with one block per CU also the first byte
    of pass two (test_large_message_later_passes' pass size)."""
    if not one_block:
        return [1, 2, 5]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [1, 2, 5, cus * 4096 // 1024]


def _edge_batch(placed):
    """One stream: in front of each (text, pos, offset) a binary message of FF
    bytes (never checked, every lane of its waves hot) that brings the text
    message's byte `pos` to the dense `offset`."""
    frames, used = [], 0
    for i, (text, pos, offset) in enumerate(placed):
        fill = offset - pos - used
        assert fill >= 0
        frames += [frame(BINARY, b"\xff" * fill, key=3 + i), frame(TEXT, text, key=0x01020304 + i)]
        used += fill + len(text)
    return mc.Batch([frames])


@pytest.mark.parametrize("one_block", [False, True], ids=["default", "1-block-per-cu"])
def test_sequences_on_wave_edges(one_block):
    """EURO and GRIN with their first byte at the dense offsets 1024 w - s,
    s = 0..4: valid; the byte above the edge made 41 (the bad position is the
    lead byte in lane 63, judged by the `post` that lane loaded); the bytes
    below the edge made 41 (a stray continuation in lane 0, judged by its own
    `pre`)."""
    c = _edge_codec(one_block)
    try:
        ws = _edge_waves(one_block)
        for seq in (uc.EURO, uc.GRIN):
            good = EDGE_BASE[:EDGE_AT] + seq + EDGE_BASE[EDGE_AT + len(seq):]
            for s in range(5):
                above = bytearray(good)
                above[EDGE_AT + s] = 0x41
                below = bytearray(good)
                below[EDGE_AT: EDGE_AT + min(s, len(seq))] = b"\x41" * min(s, len(seq))
                inside = 0 < s < len(seq)                          # the edge cuts the sequence
                for text, want in ((good, 48), (bytes(above), EDGE_AT if inside else None),
                                   (bytes(below), EDGE_AT + s if inside else None)):
                    batch = _edge_batch([(text, EDGE_AT, 1024 * w - s) for w in ws])
                    msgs, valid, result = run(c, batch, ca.UTF8_TEXT)
                    assert [int(o) + EDGE_AT + s for o in msgs["off"][1::2]] == [1024 * w for w in ws]
                    if want is not None:
                        assert valid[1::2] == [want] * len(ws), (seq, s)
                    assert result[2] == len(ws)
    finally:
        c.close()


@pytest.mark.parametrize("one_block", [False, True], ids=["default", "1-block-per-cu"])
def test_bound_just_above_a_wave_edge(one_block):
    """The batch's last message ends e = 1, 2, 3 bytes above an edge, so
    d_count[1] = 1024 w + e and lane 63's `post` is read byte by byte: a
    sequence that begins b bytes below the edge and ends whole with the
    message (b + e its length), or is cut off by the message's end (b + e
    less).  The same with msg_cap = d_count[1] exactly and BF, a continuation
    byte, behind it in d_msg: read past the bound and taken for the message's,
    it would turn a cut-off sequence into a valid one."""
    c = _edge_codec(one_block)
    try:
        for w in _edge_waves(one_block):
            for seq in (uc.EURO, uc.GRIN):
                for b in range(1, len(seq)):
                    for e in range(1, min(3, len(seq) - b) + 1):
                        text = EDGE_BASE[:EDGE_AT] + seq[: b + e]
                        want = len(text) if b + e == len(seq) else EDGE_AT
                        batch = _edge_batch([(text, EDGE_AT, 1024 * w - b)])
                        ref = model(batch)
                        used = int(ref[1][1])
                        assert used == 1024 * w + e
                        _, valid, result = run(c, batch, ca.UTF8_TEXT, ref=ref)
                        assert valid[1] == want and result[2:] == [1, len(text)], (w, seq, b, e)
                        d_msg, d_msgs, d_count = decode(c, batch)
                        torch.cuda.synchronize()
                        assert (d_msg[used:] == SENTINEL).all().item()
                        d_msg[used:] = 0xBF
                        want_valid, want_result = expected(ref[0], ref[2], ca.UTF8_TEXT, used, batch.n)
                        assert want_valid[1] == want
                        check(c, d_msg, d_msgs, d_count, ca.UTF8_TEXT, used, batch.n, want_valid, want_result)
                        assert c.sync_status() == 0
    finally:
        c.close()
