"""Record layouts shared by the C-ABI (include/wsg_capi.h) and its callers.

numpy structured dtypes whose byte layout is exactly ``wsg_send_desc``,
``wsg_recv_info``, ``wsg_msg``, ``wsg_stream_state``, ``wsg_stream_span``,
``wsg_proto_state``, ``wsg_proto_verdict`` and ``wsg_upgrade``, and the plans of
the device entry points restated on the host;
importing this module loads no native code.
"""
import numpy as np

# wsg_send_desc: one PrepareSendFrame call (reference ws.cpp:212).
SEND_DESC = np.dtype(
    [
        ("src_off", "<u8"),
        ("len", "<u8"),
        ("key", "<u4"),
        ("status", "<i4"),
        ("opcode", "u1"),
        ("mask", "u1"),
        ("_pad", "u1", (6,)),
    ]
)

# wsg_recv_info: the per-frame header arithmetic of PrepareReceiveFrame
# (reference ws.cpp:320-386).
RECV_INFO = np.dtype(
    [
        ("payload_off", "<u8"),
        ("len", "<u8"),
        ("key", "<u4"),
        ("opcode", "u1"),
        ("fin", "u1"),
        ("masked", "u1"),
        ("hdr_len", "u1"),
        ("b0", "u1"),
        ("error", "i1"),
        ("_pad", "u1", (6,)),
    ]
)

assert SEND_DESC.itemsize == 32 and RECV_INFO.itemsize == 32

# wsg_msg: one assembled message of wsg_decode_messages, what the session
# hands to its callback at a FIN frame (reference ws.cpp:411-452).
MSG = np.dtype(
    [
        ("off", "<u8"),
        ("len", "<u8"),
        ("stream", "<u4"),
        ("first_frame", "<u4"),
        ("nframes", "<u4"),
        ("status", "<i4"),
        ("kind", "u1"),
        ("opcode", "u1"),
        ("_pad", "u1", (6,)),
    ]
)

# wsg_stream_state: what a connection carries from one wsg_decode_messages
# call to the next (opcode under ASSEMBLY_REFERENCE, ahead under ASSEMBLY_RFC).
STREAM_STATE = np.dtype([("consumed", "<u4"), ("opcode", "u1"), ("_pad", "u1"), ("ahead", "<u2")])

assert MSG.itemsize == 40 and STREAM_STATE.itemsize == 8 and STREAM_STATE.fields["ahead"][1] == 6

# wsg_set_assembly's modes (include/wsg_capi.h WSG_ASSEMBLY_*): the reference's
# rule (ws.cpp:399-452), or RFC 6455 5.4 (control frames are messages of their own).
ASSEMBLY_REFERENCE, ASSEMBLY_RFC = 0, 1
AHEAD_CAP = 65535   # the most control frames STREAM_STATE.ahead counts

# wsg_stream_span: one connection's bytes in a wsg_frame_streams batch.
STREAM_SPAN = np.dtype([("off", "<u8"), ("len", "<u8"), ("consumed", "<u8"), ("need", "<u8")])

assert STREAM_SPAN.itemsize == 32

# Opcode byte values (reference include/server/ws/ws.h:33-43).
WS_FIN, WS_TEXT, WS_BINARY, WS_CLOSE, WS_PING, WS_PONG = 0x80, 0x01, 0x02, 0x08, 0x09, 0x0A

# Status codes (include/wsg_capi.h).
WSG_OK, WSG_EINVAL, WSG_ETRUNC, WSG_ENOMEM, WSG_EHIP = 0, -22, -61, -12, -5

# Callback kinds (include/wsg_capi.h WSG_CB_*).
CB_RECEIVED, CB_CLOSE, CB_PING, CB_PONG = 1, 2, 3, 4

# wsg_reply_messages' rule: the reply's first header byte by callback kind
# (0: none; REPLY_SAME: WS_FIN | the message's opcode).  ECHO_REPLY is the
# reference echo server: onWSReceived -> SendBinaryAsync
# (performance/ws_echo_server.cpp:23-26), onWSPing -> SendPongAsync
# (ws_session.h:99-101), nothing sent on a close or a pong.
REPLY_SAME = 0xFF
ECHO_REPLY = (0, WS_FIN | WS_BINARY, 0, WS_FIN | WS_PONG, 0)


def key_from_bytes(b):
    """_ws_send_mask[0..3] -> the little-endian uint32 the ABI carries."""
    b = bytes(b)
    return b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24


def frame_size(opcode, mask, length, status=0):
    """Bytes PrepareSendFrame emits (reference ws.cpp:215-252)."""
    prefix = (opcode & WS_CLOSE) == WS_CLOSE and (length > 0 or status != 0)
    body = length + (2 if prefix else 0)
    hdr = 2 if body < 126 else 4 if body < 65536 else 10
    return hdr + (4 if mask else 0) + body


def frame_sizes(desc):
    """frame_size over a SEND_DESC array, vectorized (uint64 per frame)."""
    op = desc["opcode"].astype(np.uint64)
    length = desc["len"].astype(np.uint64)
    prefix = ((op & WS_CLOSE) == WS_CLOSE) & ((length > 0) | (desc["status"] != 0))
    body = length + np.where(prefix, 2, 0).astype(np.uint64)
    hdr = np.where(body < 126, 2, np.where(body < 65536, 4, 10)).astype(np.uint64)
    return hdr + np.where(desc["mask"] != 0, 4, 0).astype(np.uint64) + body


U64_MAX = 2**64 - 1


def bad_spans(wire_len, spans):
    """Which spans wsg_frame_streams refuses (WSG_EINVAL, no frames): one that
    runs past the wire, or that starts before the end of the span before it
    where that one lies inside the wire."""
    spans = np.asarray(spans, dtype=STREAM_SPAN)
    bad = np.zeros(len(spans), dtype=bool)
    prev_end = None                                   # end of span j - 1 if it lies inside the wire
    for j in range(len(spans)):
        off, length = int(spans["off"][j]), int(spans["len"][j])
        inside = off + length <= wire_len             # Python integers: no wrap
        bad[j] = not inside or (prev_end is not None and off < prev_end)
        prev_end = off + length if inside else None
    return bad


def frame_plan(wire, spans):
    """wsg_frame_streams restated on the host over wsg_header_unpack: the
    whole frames of every stream ``wire[off, off + len)``.

    ``spans``: STREAM_SPAN records (off and len are read).  Returns
    (frame_start, stream_first, spans_out, count): the frames' wire offsets
    (uint64), the exclusive prefix of the streams' frame counts (n_streams +
    1), the spans with consumed and need filled in, and count = [frames, sum
    of consumed].  A refused span (bad_spans) has no frames, consumed 0 and
    need 0."""
    from . import _np_ptr, lib                        # the ABI's host parser; importing layout loads nothing

    unpack = lib().wsg_header_unpack
    wire = np.ascontiguousarray(wire, dtype=np.uint8)
    data = wire.tobytes()
    out = np.array(np.asarray(spans, dtype=STREAM_SPAN), copy=True)
    out["consumed"] = 0
    out["need"] = 0
    bad = bad_spans(len(data), out)
    info = np.zeros(1, dtype=RECV_INFO)
    info_p = _np_ptr(info)
    starts, first = [], [0]
    for j in range(len(out)):
        pos = int(out["off"][j])
        end = pos + int(out["len"][j])
        need = 0
        while not bad[j]:
            rem = end - pos
            if rem < 2:
                need = 2 if rem else 0
                break
            head = data[pos: min(pos + 14, end)]
            if unpack(head, len(head), info_p) != 0:  # incomplete: its length is known from the second byte
                assert unpack(head + bytes(14 - len(head)), 14, info_p) == 0
                need = int(info["hdr_len"][0])
                break
            size = int(info["hdr_len"][0]) + int(info["len"][0])
            if size > rem:
                need = min(size, U64_MAX)
                break
            starts.append(pos)
            pos += size
        if not bad[j]:
            out["consumed"][j] = pos - int(out["off"][j])
            out["need"][j] = need
        first.append(len(starts))
    count = np.array([len(starts), int(out["consumed"].astype(object).sum())], dtype=np.uint64)
    return np.array(starts, dtype=np.uint64), np.array(first, dtype=np.uint64), out, count


def _rfc_message_plan(info, stream_first, state, payload, ahead_cap):
    """message_plan under ASSEMBLY_RFC: one sequential walk per stream."""
    n_streams = len(stream_first) - 1
    new_state = np.zeros(n_streams, dtype=STREAM_STATE)
    seed = np.zeros(n_streams, dtype=STREAM_STATE) if state is None else np.asarray(state, dtype=STREAM_STATE)
    kinds = {WS_CLOSE: CB_CLOSE, WS_PING: CB_PING, WS_PONG: CB_PONG}
    msgs, used = [], 0

    def bytes_of(k):
        return bytes(payload[int(info["payload_off"][k]):][:int(info["len"][k])])

    def deliver(j, first, last, frames, opcode, kind):
        nonlocal used
        size = int(sum(int(info["len"][k]) for k in frames))
        m = np.zeros((), dtype=MSG)
        m["off"], m["len"], m["stream"], m["first_frame"], m["nframes"] = used, size, j, first, last - first + 1
        m["kind"], m["opcode"] = kind, opcode
        if opcode == WS_CLOSE:
            m["status"] = 1000
            if size >= 2:                             # the status leaves the callback's data
                m["off"], m["len"] = used + 2, size - 2
                m["status"] = 0
                if payload is not None:
                    head = bytes_of(first)
                    m["status"] = head[0] << 8 | head[1]
        msgs.append(m)
        used += size

    for j in range(n_streams):
        lo, hi = int(stream_first[j]), int(stream_first[j + 1])
        ahead_in = int(seed["ahead"][j])
        run, first_run, rank, held, data, opcode = None, True, 0, [], [], 0
        for i in range(lo, hi):
            op, fin = int(info["opcode"][i]), bool(info["fin"][i])
            if info["error"][i] or (op & 8 and not fin):
                continue                              # in no message, ends none
            if op & 8:
                if run is None:
                    deliver(j, i, i, [i], op, kinds.get(op, 0))
                    continue
                r, rank = rank, rank + 1
                if first_run and r < ahead_in:
                    continue                          # an earlier call delivered it
                if r < ahead_cap:
                    deliver(j, i, i, [i], op, kinds.get(op, 0))
                else:
                    held.append(i)                    # past what `ahead` can count: with the run's FIN frame
                continue
            if run is None:
                run, rank, held, data, opcode = i, 0, [], [], 0
            data.append(i)
            opcode = op or opcode
            if fin:
                for c in held:
                    deliver(j, c, c, [c], int(info["opcode"][c]), kinds.get(int(info["opcode"][c]), 0))
                deliver(j, run, i, data, opcode, CB_RECEIVED if opcode in (WS_TEXT, WS_BINARY) else 0)
                run, first_run = None, False
        if run is None:
            new_state["consumed"][j] = hi - lo
        else:
            new_state["consumed"][j] = run - lo
            new_state["ahead"][j] = min(rank, ahead_cap)
    table = np.array(msgs, dtype=MSG) if msgs else np.zeros(0, dtype=MSG)
    return table, np.array([len(msgs), used], dtype=np.uint64), new_state


def message_frames(info, msgs, assembly=ASSEMBLY_REFERENCE):
    """Per message of a message_plan table, the frames whose payloads make its
    buffer, in order: every frame of its span, or under ASSEMBLY_RFC a control
    frame alone, else the span's data frames without an error."""
    info = np.asarray(info, dtype=RECV_INFO)
    out = []
    for m in np.asarray(msgs, dtype=MSG):
        span = range(int(m["first_frame"]), int(m["first_frame"]) + int(m["nframes"]))
        if assembly == ASSEMBLY_RFC and not int(m["opcode"]) & 8:
            span = [k for k in span if not int(info["opcode"][k]) & 8 and not info["error"][k]]
        out.append(list(span))
    return out


def message_plan(info, stream_first, state=None, payload=None, assembly=ASSEMBLY_REFERENCE, ahead_cap=AHEAD_CAP):
    """The plan pass of wsg_decode_messages restated on the host: which
    frames make which messages (reference ws.cpp:399-452; ``assembly`` =
    ASSEMBLY_RFC: RFC 6455 5.4, the walk include/wsg_capi.h states, where the
    state's ``ahead`` is read and written, its opcode written as 0, and
    ``ahead_cap`` is the most it counts: 65535 on the device).

    ``info``: RECV_INFO of the batch's frames; ``stream_first``: n_streams + 1
    frame indices, stream j's frames are [stream_first[j], stream_first[j+1])
    in arrival order; ``state``: STREAM_STATE per stream (None: zeros).
    Returns (msgs, count, new_state): the MSG table in the order of the FIN
    frames, count = [messages, bytes of the dense message buffer], and each
    stream's frames consumed and _ws_opcode for the next call.

    A close message's status is the first two bytes of its buffer
    (ws.cpp:435-439), so it needs bytes: ``payload`` is the batch with its
    payloads unmasked where they sit (wsg_decode_batch's output); without it
    such a status is left 0.
    """
    info = np.asarray(info, dtype=RECV_INFO)
    stream_first = np.asarray(stream_first, dtype=np.int64)
    if assembly == ASSEMBLY_RFC:
        return _rfc_message_plan(info, stream_first, state, payload, ahead_cap)
    n_streams = len(stream_first) - 1
    new_state = np.zeros(n_streams, dtype=STREAM_STATE)
    if state is not None:
        new_state["opcode"] = np.asarray(state, dtype=STREAM_STATE)["opcode"]
    kinds = {WS_TEXT: CB_RECEIVED, WS_BINARY: CB_RECEIVED, WS_CLOSE: CB_CLOSE, WS_PING: CB_PING, WS_PONG: CB_PONG}
    msgs, used = [], 0
    for j in range(n_streams):
        lo, hi = int(stream_first[j]), int(stream_first[j + 1])
        fins = [i for i in range(lo, hi) if info["fin"][i]]
        opcode = int(new_state["opcode"][j])          # _ws_opcode: sticky, never reset (ws.cpp:326)
        first = lo                                    # the open message's first frame
        for i in range(lo, fins[-1] + 1 if fins else lo):   # frames after the last FIN frame: the tail
            opcode = int(info["opcode"][i]) or opcode
            if not info["fin"][i]:
                continue
            frames = range(first, i + 1)              # every frame since the previous FIN, control frames too
            size = int(sum(int(info["len"][k]) for k in frames))
            m = np.zeros((), dtype=MSG)
            m["off"], m["len"], m["stream"], m["first_frame"], m["nframes"] = used, size, j, first, len(frames)
            m["kind"], m["opcode"] = kinds.get(opcode, 0), opcode
            if opcode == WS_CLOSE:
                m["status"] = 1000
                if size >= 2:                         # the status leaves the callback's data
                    m["off"], m["len"] = used + 2, size - 2
                    m["status"] = 0
                    if payload is not None:
                        head = b"".join(bytes(payload[int(info["payload_off"][k]):][:int(info["len"][k])])[:2]
                                        for k in frames)[:2]
                        m["status"] = head[0] << 8 | head[1]
            msgs.append(m)
            used += size
            first = i + 1
        new_state["consumed"][j] = first - lo
        new_state["opcode"][j] = opcode
    table = np.array(msgs, dtype=MSG) if msgs else np.zeros(0, dtype=MSG)
    return table, np.array([len(msgs), used], dtype=np.uint64), new_state


def reply_plan(msgs, reply_op, mask, send_keys=None, n_streams=None):
    """The sizes and offsets of wsg_reply_messages' output (not its bytes).

    ``msgs``: a message_plan table; ``reply_op``: five bytes indexed by CB_*
    (entry 0 ignored); ``send_keys``: one per stream, or None (keys do not
    change a size); ``n_streams``: defaults to len(send_keys), else to the
    last stream of the table + 1.  Returns (reply_off, stream_reply, count):
    len(msgs) + 1 and n_streams + 1 offsets into the reply wire, and count =
    [reply bytes, reply frames]."""
    msgs = np.asarray(msgs, dtype=MSG)
    if n_streams is None:
        n_streams = len(send_keys) if send_keys is not None else int(msgs["stream"].max()) + 1 if len(msgs) else 0
    sizes = np.zeros(len(msgs), dtype=np.uint64)
    for q, m in enumerate(msgs):
        kind = int(m["kind"])
        op = int(reply_op[kind]) if kind else 0
        op = WS_FIN | int(m["opcode"]) if op == REPLY_SAME else op
        if op:   # a close reply carries the status and no data
            sizes[q] = frame_size(op, mask, 0, int(m["status"])) if kind == CB_CLOSE else \
                frame_size(op, mask, int(m["len"]))
    reply_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    # messages are stream-major: stream j's begin at the first record of a stream >= j
    stream_reply = reply_off[np.searchsorted(msgs["stream"], np.arange(n_streams + 1))]
    return reply_off, stream_reply, np.array([int(reply_off[-1]), int((sizes > 0).sum())], dtype=np.uint64)


# wsg_check_utf8's `which` bits (include/wsg_capi.h WSG_UTF8_*).
UTF8_TEXT, UTF8_CLOSE, UTF8_EVERY = 1, 2, 4


def _utf8_len(b):
    """Length a non-continuation byte declares (0: never valid)."""
    return 1 if b < 0x80 else 0 if b < 0xC2 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4 if b < 0xF5 else 0


def _utf8_bad_at(b, i):
    """The position-local rule of csrc/wsg_utf8.h: is position i of the byte
    string b bad?  Every byte outside b counts as 00."""
    def at(j):
        return b[j] if 0 <= j < len(b) else 0

    def cont(x):
        return x & 0xC0 == 0x80

    if cont(b[i]):
        for k in (1, 2, 3):
            if not cont(at(i - k)):
                return _utf8_len(at(i - k)) <= k
        return True
    size = _utf8_len(b[i])
    if size <= 1:
        return size == 0
    lead, second = b[i], at(i + 1)
    lo = 0xA0 if lead == 0xE0 else 0x90 if lead == 0xF0 else 0x80
    hi = 0x9F if lead == 0xED else 0x8F if lead == 0xF4 else 0xBF
    if not lo <= second <= hi:
        return True
    return any(not cont(at(i + k)) for k in range(2, size))


def utf8_valid_up_to(data):
    """Length of the longest well-formed UTF-8 prefix of ``data`` (RFC 3629):
    the smallest bad position, by the position-local rule (no decoder)."""
    b = bytes(data)
    for i in range(len(b)):
        if b[i] >= 0x80 and _utf8_bad_at(b, i):
            return i
    return len(b)


def utf8_plan(msgs, msg_bytes, which, msg_cap=None):
    """wsg_check_utf8 restated on the host over a MSG table and the dense
    message bytes it describes (``msg_bytes`` is d_msg[0, d_count[1])).

    Returns (valid, result): valid[m] = valid_up_to of message m's data when
    it is selected by ``which`` (UTF8_* bits, from kind and opcode alone) and
    lies inside min(msg_cap, len(msg_bytes)), its len otherwise; result =
    [checked messages that are invalid, the lowest of them or 2**64 - 1,
    messages checked, bytes checked]."""
    msgs = np.asarray(msgs, dtype=MSG)
    buf = np.asarray(msg_bytes, dtype=np.uint8).tobytes()
    bound = len(buf) if msg_cap is None else min(int(msg_cap), len(buf))
    valid = np.zeros(len(msgs), dtype=np.uint64)
    invalid, lowest, checked, nbytes = 0, U64_MAX, 0, 0
    for m, r in enumerate(msgs):
        off, size, kind, opcode = int(r["off"]), int(r["len"]), int(r["kind"]), int(r["opcode"])
        valid[m] = size
        selected = bool(which & UTF8_EVERY) or (bool(which & UTF8_TEXT) and kind == CB_RECEIVED and opcode == WS_TEXT) \
            or (bool(which & UTF8_CLOSE) and kind == CB_CLOSE)
        if not selected or off + size > bound:
            continue
        checked += 1
        nbytes += size
        valid[m] = utf8_valid_up_to(buf[off: off + size])
        if int(valid[m]) < size:
            invalid += 1
            lowest = min(lowest, m)
    return valid, np.array([invalid, lowest, checked, nbytes], dtype=np.uint64)


def utf8_wire_plan(info, stream_first, state, payload, which, assembly=ASSEMBLY_REFERENCE):
    """wsg_check_utf8_wire restated on the host: message_plan over the frame
    table, the dense message bytes gathered from ``payload`` (the batch with
    its payloads unmasked where they sit, wsg_decode_batch's output) and
    utf8_plan over them.  Returns (msgs, count, valid, result); ``state`` is
    only read."""
    info = np.asarray(info, dtype=RECV_INFO)
    msgs, count, new_state = message_plan(info, stream_first, state, payload, assembly=assembly)
    sf = np.asarray(stream_first, dtype=np.int64)
    buf = np.asarray(payload, dtype=np.uint8)
    dense = []
    if assembly == ASSEMBLY_RFC:   # the messages' frames, in the messages' order
        delivered = [i for frames in message_frames(info, msgs, assembly) for i in frames]
    else:                          # every stream's consumed frames, in order
        delivered = [i for j in range(len(sf) - 1) for i in range(int(sf[j]), int(sf[j]) + int(new_state["consumed"][j]))]
    for i in delivered:
        dense.append(buf[int(info["payload_off"][i]): int(info["payload_off"][i]) + int(info["len"][i])])
    dense = np.concatenate(dense) if dense else np.zeros(0, dtype=np.uint8)
    assert len(dense) == int(count[1])
    valid, result = utf8_plan(msgs, dense, which)
    return msgs, count, valid, result


# wsg_check_protocol (include/wsg_capi.h): the per-stream state, the verdict
# and the WSG_PV_* / WSG_PROTO_* constants.
PROTO_STATE = np.dtype([("bytes", "<u8"), ("open", "u1"), ("_pad", "u1", (7,))])
PROTO_VERDICT = np.dtype([("code", "u1"), ("_pad", "u1"), ("status", "<u2"), ("frame", "<u4")])

assert PROTO_STATE.itemsize == 16 and PROTO_VERDICT.itemsize == 8

(PV_CLOSED, PV_FRAME, PV_RSV, PV_OPCODE, PV_MASK, PV_CTRL_FRAGMENT, PV_CTRL_LONG, PV_CONT, PV_DATA, PV_CLOSE_LEN,
 PV_CLOSE_CODE, PV_TOO_BIG) = range(1, 13)
PV_NONE = 0xFF
PROTO_ANY, PROTO_SERVER, PROTO_CLIENT = 0, 1, 2


def protocol_plan(info, stream_first, proto_in, role, max_message, wire, consumed=None):
    """wsg_check_protocol restated on the host in vectorised numpy: no loop
    over frames or streams; a frame's state comes from running maxima (the
    last frame that set the byte count, the last that set `open`) and a
    running sum, as the kernels' comes from a scan.

    ``info``: RECV_INFO of the batch's frames; ``stream_first``: n_streams + 1
    frame indices; ``proto_in``: PROTO_STATE per stream (None: zeros);
    ``wire``: the bytes payload_off indexes (read for close statuses only);
    ``consumed``: per stream, as STREAM_STATE.consumed (None: the state after
    each stream's last frame).  Returns (verdict, proto_out, result):
    PROTO_VERDICT and PROTO_STATE per stream and result = [streams whose
    terminal frame is a violation, the lowest of them or 2**64 - 1, streams
    closed cleanly]."""
    info = np.asarray(info, dtype=RECV_INFO)
    n = len(info)
    sf = np.minimum(np.asarray(stream_first, dtype=np.int64), n)
    ns = len(sf) - 1
    seed = np.zeros(ns, dtype=PROTO_STATE)
    if proto_in is not None:
        seed["bytes"] = np.asarray(proto_in, dtype=PROTO_STATE)["bytes"]
        seed["open"] = np.asarray(proto_in, dtype=PROTO_STATE)["open"] != 0
    verdict = np.frombuffer(b"\xff" * (8 * ns), dtype=PROTO_VERDICT).copy()
    proto_out = seed.copy()
    result = np.array([0, U64_MAX, 0], dtype=np.uint64)
    if ns == 0 or n == 0:
        return verdict, proto_out, result
    idx = np.arange(n, dtype=np.int64)
    sidx = np.maximum(np.searchsorted(sf[:ns], idx, side="right") - 1, 0)   # the last j with sf[j] <= i
    head = sf[sidx]
    op = info["opcode"].astype(np.int64)
    fin = info["fin"] != 0
    masked = info["masked"] != 0
    error = info["error"] != 0
    rsv = (info["b0"] & 0x70) != 0
    length = info["len"].astype(object)                                       # Python integers: sums do not wrap
    keep = error | (op > 2)
    sets = ~keep & (op != 0)
    adds = ~keep & (op == 0)

    def last_before(flag):
        """Per frame: the last flagged frame in front of it in its stream, -1 when there is none."""
        inc = np.maximum.accumulate(np.where(flag, idx, -1))
        ex = np.concatenate([[-1], inc[:-1]])
        return np.where(ex >= head, ex, -1)

    p_set, p_any = last_before(sets), last_before(~keep)
    add_sum = np.concatenate([[0], np.cumsum(np.where(adds, length, 0).astype(object))])   # of the frames before k
    base = np.where(p_set >= 0, length[np.maximum(p_set, 0)], seed["bytes"][sidx].astype(object))
    since = np.where(p_set >= 0, p_set + 1, head)
    before = np.minimum(base + (add_sum[idx] - add_sum[since]), U64_MAX)
    open_before = np.where(p_any >= 0, ~fin[np.maximum(p_any, 0)], seed["open"][sidx] != 0)
    after = np.where(keep, before, np.where(sets, length, np.minimum(before + length, U64_MAX)))
    open_after = np.where(keep, open_before, ~fin)

    # the close status on the wire
    wire = np.asarray(wire, dtype=np.uint8)
    po = info["payload_off"]
    has_status = (op == WS_CLOSE) & (info["len"] >= 2) & (len(wire) >= 2) & (po <= np.uint64(max(len(wire) - 2, 0)))
    carried = np.zeros(n, dtype=np.int64)                                     # (two bytes past the wire: read as 0)
    at = po[has_status].astype(np.int64)
    key = info["key"][has_status].astype(np.int64) * masked[has_status]
    carried[has_status] = ((wire[at].astype(np.int64) ^ (key & 0xFF)) << 8) | (wire[at + 1] ^ ((key >> 8) & 0xFF))
    status_ok = ((carried >= 1000) & (carried <= 1003)) | ((carried >= 1007) & (carried <= 1014)) | \
        ((carried >= 3000) & (carried <= 4999))

    control = (op & 8) != 0
    reserved = ((op >= 3) & (op <= 7)) | (op >= 0xB)
    data = op <= 2
    rules = [
        (error, PV_FRAME),
        (rsv, PV_RSV),
        (reserved, PV_OPCODE),
        (~masked if role == PROTO_SERVER else masked if role == PROTO_CLIENT else np.zeros(n, dtype=bool), PV_MASK),
        (control & ~fin, PV_CTRL_FRAGMENT),
        (control & (length > 125), PV_CTRL_LONG),
        ((op == 0) & ~open_before, PV_CONT),
        (data & (op != 0) & open_before, PV_DATA),
        ((op == WS_CLOSE) & (length == 1), PV_CLOSE_LEN),
        ((op == WS_CLOSE) & (length >= 2) & ~status_ok, PV_CLOSE_CODE),
        (data & (after > max_message) if max_message else np.zeros(n, dtype=bool), PV_TOO_BIG),
        (op == WS_CLOSE, PV_CLOSED),
    ]
    code = np.select([r[0].astype(bool) for r in rules], [r[1] for r in rules], 0)
    status = np.where(code == PV_TOO_BIG, 1009, np.where(code == PV_CLOSED, np.where(length == 0, 1005, carried), 1002))

    judged = np.nonzero(code)[0]                                              # ascending: a stream's first comes first
    streams, first = np.unique(sidx[judged], return_index=True)
    term = judged[first]
    verdict["code"][streams] = code[term]
    verdict["_pad"][streams] = 0
    verdict["status"][streams] = status[term].astype(np.int64)
    verdict["frame"][streams] = term

    start, end = sf[:-1], np.maximum(sf[1:], sf[:-1])
    target = end if consumed is None else start + np.asarray(consumed, dtype=np.int64)
    has = (target > start) & (target <= end)
    last = np.maximum(target - 1, 0)[has]
    proto_out["bytes"][has] = after[last].astype(np.uint64)
    proto_out["open"][has] = open_after[last].astype(bool)

    bad = verdict["code"][streams] >= PV_FRAME
    result[0] = int(bad.sum())
    if bad.any():
        result[1] = int(streams[bad].min())
    result[2] = int((verdict["code"][streams] == PV_CLOSED).sum())
    return verdict, proto_out, result


# wsg_reply_checked / wsg_utf8_verdicts (include/wsg_capi.h).
PV_UTF8 = 13
NO_VERDICT = np.frombuffer(b"\xff" * 8, dtype=PROTO_VERDICT)[0]


def _verdict_words(verdict):
    """PROTO_VERDICT records as the little-endian words the kernels order them by."""
    return np.ascontiguousarray(np.asarray(verdict, dtype=PROTO_VERDICT)).view("<u8").copy()


def merge_verdicts(verdict, also, stream_first):
    """wsg_reply_checked's effective verdicts: ``verdict`` (the protocol's,
    PROTO_VERDICT per stream) with ``also`` (None: none) taken where it names
    a frame of its stream [stream_first[j], stream_first[j+1]) and comes
    first: a lower frame, or the same frame where the protocol's code is
    PV_CLOSED and the other's >= 2.  An all-0xFF entry means none."""
    out = np.array(np.asarray(verdict, dtype=PROTO_VERDICT), copy=True)
    if also is None or len(out) == 0:
        return out
    also = np.asarray(also, dtype=PROTO_VERDICT)
    sf = np.asarray(stream_first, dtype=np.int64)
    a, v = _verdict_words(also), _verdict_words(out)
    frame = also["frame"].astype(np.int64)
    usable = (a != U64_MAX) & (frame >= sf[:-1]) & (frame < sf[1:])
    vf = out["frame"].astype(np.int64)
    take = usable & ((frame < vf) | ((frame == vf) & (out["code"] == PV_CLOSED) & (also["code"] >= PV_FRAME)))
    v[take] = a[take]
    return v.view(PROTO_VERDICT)


def utf8_verdicts(msgs, valid, which, n_streams):
    """wsg_utf8_verdicts: per stream, all 0xFF or {PV_UTF8, 1007, the FIN
    frame} of its first message that ``which`` selects (utf8_plan's rule)
    and whose valid[m] < len."""
    msgs = np.asarray(msgs, dtype=MSG)
    words = np.full(n_streams, U64_MAX, dtype=np.uint64)
    kind, opcode = msgs["kind"], msgs["opcode"]
    selected = np.full(len(msgs), bool(which & UTF8_EVERY))
    if which & UTF8_TEXT:
        selected |= (kind == CB_RECEIVED) & (opcode == WS_TEXT)
    if which & UTF8_CLOSE:
        selected |= kind == CB_CLOSE
    bad = selected & (np.asarray(valid, dtype=np.uint64)[: len(msgs)] < msgs["len"]) & (msgs["stream"] < n_streams)
    fin = msgs["first_frame"].astype(np.uint64) + msgs["nframes"].astype(np.uint64) - np.uint64(1)
    word = np.uint64(PV_UTF8) | (np.uint64(1007) << np.uint64(16)) | (fin << np.uint64(32))
    np.minimum.at(words, msgs["stream"][bad].astype(np.int64), word[bad])
    return words.view(PROTO_VERDICT)


def validated_verdicts(msgs, valid, which, also, stream_first):
    """The d_also that wsg_reply_validated hands to its reply kernels: per
    stream the UTF-8 verdict (utf8_verdicts), the caller's ``also`` entry
    (None: none) where that is not all 0xFF and names a frame of the stream,
    or the lower of the two as one little-endian word.  An entry outside its
    stream's range is dropped before the comparison."""
    sf = np.asarray(stream_first, dtype=np.int64)
    n_streams = len(sf) - 1
    words = _verdict_words(utf8_verdicts(msgs, valid, which, n_streams)) if n_streams else np.zeros(0, dtype="<u8")
    if also is not None:
        given = np.asarray(also, dtype=PROTO_VERDICT)
        a = _verdict_words(given)
        for j in range(n_streams):
            if int(a[j]) != U64_MAX and int(sf[j]) <= int(given["frame"][j]) < int(sf[j + 1]):
                words[j] = min(int(words[j]), int(a[j]))
    return words.view(PROTO_VERDICT)


def checked_reply_plan(msgs, verdict, reply_op, mask, send_keys=None, n_streams=None):
    """The sizes and offsets of wsg_reply_checked's output (not its bytes).

    ``msgs``: a message_plan table; ``verdict``: the effective PROTO_VERDICT
    per stream (merge_verdicts); the rest as reply_plan.  A message whose FIN
    frame lies in front of its stream's terminal frame is sized as reply_plan
    sizes it, any other gets nothing, and the terminal frame holds the close
    frame (status 1005 sent as 1000).  Returns (reply_off, stream_reply,
    close_off, count): reply_off[m] the reply bytes, close frames included,
    of the frames in front of message m's FIN frame (len(msgs) + 1 entries,
    the last the total); n_streams + 1 stream offsets; per stream the close
    frame's offset or 2**64 - 1; count = [reply bytes, reply frames (both with
    the close frames), close frames]."""
    msgs = np.asarray(msgs, dtype=MSG)
    verdict = np.asarray(verdict, dtype=PROTO_VERDICT)
    if n_streams is None:
        n_streams = len(verdict)
    sizes = np.diff(reply_plan(msgs, reply_op, mask, send_keys, n_streams=n_streams)[0].astype(np.int64))
    fin = msgs["first_frame"].astype(np.int64) + msgs["nframes"].astype(np.int64) - 1
    has = _verdict_words(verdict) != U64_MAX if n_streams else np.zeros(0, dtype=bool)
    term = np.where(has, verdict["frame"].astype(np.int64), np.int64(2**62))
    if len(msgs):
        sizes = np.where(fin < term[msgs["stream"]], sizes, 0)
    status = np.where(verdict["status"] == 1005, 1000, verdict["status"]).astype(np.int64)
    closing = np.nonzero(has)[0]
    close_size = np.array([frame_size(WS_FIN | WS_CLOSE, mask, 0, int(status[j])) for j in closing], dtype=np.int64)
    close_frame = term[closing]
    # bytes that belong to frames in front of frame k: replies by their FIN frame, close frames by their terminal one
    at = np.concatenate([fin, close_frame])
    size = np.concatenate([sizes, close_size]).astype(np.int64)
    order = np.argsort(at, kind="stable")
    at_sorted, cum = at[order], np.concatenate([[0], np.cumsum(size[order])])

    def before(k):
        return cum[np.searchsorted(at_sorted, k, side="left")]

    total = int(cum[-1])
    reply_off = np.concatenate([before(fin), [total]]).astype(np.uint64)
    # stream j's first frame: its first message's first frame or its terminal frame, whichever is there;
    # messages are stream-major and frames too, so the bytes in front of stream j are those of lower streams
    per_stream = np.zeros(n_streams + 1, dtype=np.int64)
    if len(msgs):
        np.add.at(per_stream, msgs["stream"].astype(np.int64) + 1, sizes)
    np.add.at(per_stream, closing + 1, close_size)
    stream_reply = np.cumsum(per_stream).astype(np.uint64)
    close_off = np.full(n_streams, U64_MAX, dtype=np.uint64)
    close_off[closing] = before(close_frame).astype(np.uint64)
    count = np.array([total, int((sizes > 0).sum()) + len(closing), len(closing)], dtype=np.uint64)
    return reply_off, stream_reply, close_off, count


# ---- relays (wsg_relay_validated) ---------------------------------------------
# The reference's chat server (examples/ws_chat_server.cpp:35-46): every text
# message goes to every session, a ping is answered to its sender.
CHAT_REPLY = (0, 0, 0, WS_FIN | WS_PONG, 0)
CHAT_RELAY = (0, WS_FIN | WS_TEXT, 0, 0, 0)


def relay_tables_bad(n_streams, order=None, group_first=None):
    """The lowest offending position of wsg_relay_validated's room tables, or
    None when they keep their rules: a position p whose ``order`` entry is
    >= n_streams or names a stream that a lower position names; behind every
    position, n_streams + g for an entry g of ``group_first`` that is not 0 at
    g == 0, lies below entry g - 1, or is not n_streams at the last entry."""
    if order is not None:
        seen = set()
        for p, j in enumerate(np.asarray(order).tolist()[:n_streams]):
            if j >= n_streams or j in seen:
                return p
            seen.add(j)
    if group_first is not None:
        gf = np.asarray(group_first).tolist()
        for g, v in enumerate(gf):
            if (g == 0 and v != 0) or (g > 0 and v < gf[g - 1]) or (g == len(gf) - 1 and v != n_streams):
                return n_streams + g
    return None


def relay_plan(msgs, verdict, relay_op, order=None, group_first=None):
    """The sizes and offsets of wsg_relay_validated's relay side (not its bytes).

    ``msgs``: a message_plan table; ``verdict``: the effective PROTO_VERDICT
    per stream (n_streams of them); ``relay_op``: five bytes indexed by CB_*
    (entry 0 ignored), with reply_op's meaning; ``order``: a permutation of
    the stream indices, None the identity; ``group_first``: n_groups + 1
    positions, None one room of everyone.  A message is relayed when
    relay_op names its kind and the frame that ends it lies in front of its
    stream's terminal frame; its frame is unmasked.  Returns (relay_off,
    group_relay, count): per message the start of its relay frame in d_relay
    or 2**64 - 1, n_groups + 1 offsets (group g's range, the last the total),
    count = [relay bytes, relay frames, 0].  When the tables break their rules
    (relay_tables_bad) nothing is relayed: all 2**64 - 1, all 0, [0, 0, 0]."""
    msgs = np.asarray(msgs, dtype=MSG)
    verdict = np.asarray(verdict, dtype=PROTO_VERDICT)
    ns = len(verdict)
    n_groups = 1 if group_first is None else len(group_first) - 1
    relay_off = np.full(len(msgs), U64_MAX, dtype=np.uint64)
    if relay_tables_bad(ns, order, group_first) is not None:
        return relay_off, np.zeros(n_groups + 1, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    sizes = np.diff(reply_plan(msgs, relay_op, False, n_streams=ns)[0].astype(np.int64))
    last = msgs["first_frame"].astype(np.int64) + msgs["nframes"].astype(np.int64) - 1
    has = _verdict_words(verdict) != U64_MAX if ns else np.zeros(0, dtype=bool)
    term = np.where(has, verdict["frame"].astype(np.int64), np.int64(2**62))
    if len(msgs):
        sizes = np.where(last < term[msgs["stream"]], sizes, 0)
    per_stream = np.zeros(ns, dtype=np.int64)
    if len(msgs):
        np.add.at(per_stream, msgs["stream"].astype(np.int64), sizes)
    order = np.arange(ns, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    # the bytes in front of position p, and of the stream that stands there
    before_pos = np.concatenate([[0], np.cumsum(per_stream[order])]).astype(np.int64)
    base = np.zeros(ns, dtype=np.int64)
    base[order] = before_pos[:-1]
    if len(msgs):   # messages are stream-major: a stream's relayed messages follow its base back to back
        before = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        stream = msgs["stream"].astype(np.int64)
        first = np.searchsorted(stream, np.arange(ns))
        at = base[stream] + before[:-1] - before[np.minimum(first, len(msgs))[stream]]
        relay_off = np.where(sizes > 0, at, -1).astype(np.int64).view(np.uint64)
    gf = np.array([0, ns], dtype=np.int64) if group_first is None else np.asarray(group_first).astype(np.int64)
    count = np.array([int(before_pos[-1]), int((sizes > 0).sum()), 0], dtype=np.uint64)
    return relay_off, before_pos[gf].astype(np.uint64), count


# ---- the upgrade handshake (wsg_upgrade_streams) -----------------------------
UPGRADE_DTYPE = np.dtype([("key_off", "<u8"), ("url_off", "<u8"), ("key_len", "<u4"), ("url_len", "<u4"),
                          ("resp_len", "<u4"), ("status", "<u2"), ("code", "u1"), ("_pad", "u1")])
(UP_INCOMPLETE, UP_ACCEPTED, UP_BAD_HTTP, UP_BAD_CONNECTION, UP_BAD_UPGRADE, UP_EMPTY_KEY, UP_BAD_VERSION, UP_MISSING,
 UP_NOT_GET, UP_NOT_WEBSOCKET, UP_TOO_LONG) = range(11)
UPGRADE_RESP_MAX = 196
WS_GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"
_UP_TEXT = {
    UP_BAD_HTTP: b"Invalid HTTP request",
    UP_BAD_CONNECTION: b"Invalid WebSocket handshaked request: 'Connection' header value must be 'Upgrade' or "
                       b"'keep-alive, Upgrade'",
    UP_BAD_UPGRADE: b"Invalid WebSocket handshaked request: 'Upgrade' header value must be 'websocket'",
    UP_EMPTY_KEY: b"Invalid WebSocket handshaked request: 'Sec-WebSocket-Key' header value must be non empty",
    UP_BAD_VERSION: b"Invalid WebSocket handshaked request: 'Sec-WebSocket-Version' header value must be '13'",
    UP_MISSING: b"Invalid WebSocket response",
}


def ws_accept(key):
    """Base64(SHA-1(key || GUID)): the Sec-WebSocket-Accept value of ``key``."""
    import base64
    import hashlib

    return base64.b64encode(hashlib.sha1(bytes(key) + WS_GUID).digest())


def upgrade_response(code, key=b""):
    """The bytes HTTPResponse serialises for an outcome (b"" when it gets none)."""
    if code == UP_ACCEPTED:
        return (b"HTTP/1.1 101 Switching Protocols\r\nConnection: Upgrade\r\nUpgrade: websocket\r\n"
                b"Sec-WebSocket-Accept: " + ws_accept(key) + b"\r\nContent-Length: 0\r\n\r\n")
    text = _UP_TEXT.get(code)
    if text is None:
        return b""
    return (b"HTTP/1.1 400 Bad Request\r\nContent-Type: text/plain; charset=UTF-8\r\nContent-Length: %d\r\n\r\n%s"
            % (len(text), text))


def _lower(b):
    return bytes(c + 32 if 65 <= c <= 90 else c for c in b)   # ASCII only, as tolower in the C locale


def upgrade_judge(data, max_request=0):
    """One connection's first bytes as WSSession::onReceived, HTTPRequest::Parse
    and WebSocket::PerformServerUpgrade judge them.  Returns a dict: code,
    status, consumed, need, key (offset, length), url (offset, length), resp."""
    data = bytes(data)
    out = dict(code=UP_TOO_LONG if max_request and len(data) >= max_request else UP_INCOMPLETE, status=0, consumed=0,
               need=0, key=(0, 0), url=(0, 0), resp=b"")
    p = data.find(b"\r\n\r\n")
    if p < 0:
        return out
    hend = p + 4
    eol = data.find(b"\r\n")
    line = data[:eol]
    s1, s2 = line.find(b" "), line.rfind(b" ")
    bad = s1 < 0 or s1 == s2
    headers, clen, at = [], 0, eol + 2
    block_end = max(hend - 2, at)
    while not bad and at < block_end:
        e = data.find(b"\r\n", at, block_end)
        e = block_end if e < 0 else e
        ln = data[at:e]
        if ln:
            colon = ln.find(b":")
            if colon <= 0:
                bad = True
                break
            k, v = ln[:colon].strip(b" \t"), ln[colon + 1:].strip(b" \t")
            v_at = at + colon + 1 + (len(ln[colon + 1:]) - len(ln[colon + 1:].lstrip(b" \t")))
            headers.append((_lower(k), v, v_at))
            if _lower(k) == b"content-length":
                clen = 0
                for c in v:
                    if not 48 <= c <= 57:
                        bad = True
                        break
                    clen = (clen * 10 + c - 48) % 2**64
        at = e + 2
    if bad:
        out.update(code=UP_BAD_HTTP, status=400, consumed=hend, resp=upgrade_response(UP_BAD_HTTP))
        return out
    if len(data) - hend < clen:
        out["need"] = min(hend + clen, U64_MAX)
        return out
    out.update(code=UP_NOT_GET, consumed=hend + clen, url=(s1 + 1, s2 - s1 - 1))
    if line[:s1] != b"GET":
        return out
    seen, fail, key = set(), 0, None
    for k, v, v_at in headers:
        if k == b"connection":
            squeezed = bytes(c for c in v if c not in b" \t\n\v\f\r")
            if _lower(v) != b"upgrade" and _lower(squeezed) != b"keep-alive,upgrade":
                fail = UP_BAD_CONNECTION
        elif k == b"upgrade":
            if _lower(v) != b"websocket":
                fail = UP_BAD_UPGRADE
        elif k == b"sec-websocket-key":
            if not v:
                fail = UP_EMPTY_KEY
            else:
                key = (v_at, len(v))
        elif k == b"sec-websocket-version":
            if v != b"13":
                fail = UP_BAD_VERSION
        else:
            continue
        if fail:
            break
        seen.add(k)
    if key is not None:
        out["key"] = key
    if not seen:                 # whatever failed: none of the four in front of it
        code = UP_NOT_WEBSOCKET
    elif len(seen) != 4:
        code = fail or UP_MISSING
    else:                        # all four in front of a failing header: that one no longer counts
        code = UP_ACCEPTED
    resp = upgrade_response(code, data[key[0]:key[0] + key[1]] if key else b"")
    out.update(code=code, resp=resp, status=101 if code == UP_ACCEPTED else 400 if resp else 0)
    return out


def upgrade_plan(wire, spans, max_request=0):
    """wsg_upgrade_streams restated on the host: one request per stream
    ``wire[off, off + len)``.  Returns (up, consumed, need, resp_off, resp,
    count, bad): UPGRADE_DTYPE records, the spans' outputs, the exclusive
    prefix of resp_len (n_streams + 1), the response bytes in stream order,
    count = [accepted, answered with a 400, incomplete, response bytes], and
    the spans latched as WSG_EINVAL (bad_spans)."""
    wire = np.asarray(wire, dtype=np.uint8)
    spans = np.asarray(spans, dtype=STREAM_SPAN)
    ns = len(spans)
    bad = bad_spans(len(wire), spans)
    up = np.zeros(ns, dtype=UPGRADE_DTYPE)
    consumed = np.zeros(ns, dtype=np.uint64)
    need = np.zeros(ns, dtype=np.uint64)
    resp_off = np.zeros(ns + 1, dtype=np.uint64)
    resp = []
    for j in range(ns):
        if not bad[j]:
            off, length = int(spans["off"][j]), int(spans["len"][j])
            o = upgrade_judge(wire[off:off + length].tobytes(), max_request)
            u = up[j]
            u["code"], u["status"], u["resp_len"] = o["code"], o["status"], len(o["resp"])
            if o["key"][1]:
                u["key_off"], u["key_len"] = off + o["key"][0], o["key"][1]
            if o["code"] not in (UP_INCOMPLETE, UP_TOO_LONG, UP_BAD_HTTP):
                u["url_off"], u["url_len"] = off + o["url"][0], o["url"][1]
            consumed[j], need[j] = o["consumed"], o["need"]
            resp.append(o["resp"])
        resp_off[j + 1] = resp_off[j] + np.uint64(up["resp_len"][j])
    count = np.array([np.sum(up["code"] == UP_ACCEPTED), np.sum(up["status"] == 400),
                      np.sum(up["code"] == UP_INCOMPLETE), resp_off[ns]], dtype=np.uint64)
    return up, consumed, need, resp_off, np.frombuffer(b"".join(resp), dtype=np.uint8), count, bad


# ---- the client's half of the handshake (wsg_upgrade_client_streams) ---------
UPGRADE_REPLY_DTYPE = np.dtype([("accept_off", "<u8"), ("body_off", "<u8"), ("accept_len", "<u4"), ("body_len", "<u4"),
                                ("_zero", "<u4"), ("status", "<u2"), ("code", "u1"), ("_pad", "u1")])
(UC_INCOMPLETE, UC_ACCEPTED, UC_BAD_HTTP, UC_BAD_CONNECTION, UC_BAD_UPGRADE, UC_BAD_ACCEPT, UC_MISSING, UC_NOT_101,
 UC_TOO_LONG) = range(9)
_B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"

assert UPGRADE_REPLY_DTYPE.itemsize == 32


def upgrade_expect(nonce):
    """SHA-1(Base64(nonce) || GUID): the 20 bytes a client holds the decoded
    Sec-WebSocket-Accept value against."""
    import base64
    import hashlib

    nonce = bytes(nonce)
    assert len(nonce) == 16
    return hashlib.sha1(base64.b64encode(nonce) + WS_GUID).digest()


def upgrade_request(tpl, key_at, nonce):
    """wsg_upgrade_request: the template with Base64(nonce) in its 24-byte
    hole at ``key_at``."""
    import base64

    tpl, nonce = bytes(tpl), bytes(nonce)
    assert len(nonce) == 16 and 0 <= key_at and key_at + 24 <= len(tpl)
    return tpl[:key_at] + base64.b64encode(nonce) + tpl[key_at + 24:]


def _accept_ok(value, expect):
    """The value decoded as WS::Base64Decode does (a byte outside the
    alphabet is skipped, six bits a letter, a byte whenever eight are held),
    then strncmp(got, expect, min(len(got), 20))."""
    got, acc, bits = bytearray(), 0, 0
    for c in value:
        v = _B64.find(bytes([c]))
        if v < 0:
            continue
        acc = (acc << 6) | v
        bits += 6
        if bits >= 8:
            bits -= 8
            got.append((acc >> bits) & 0xFF)
    for i in range(min(len(got), 20)):
        if got[i] != expect[i]:
            return False
        if got[i] == 0:
            return True
    return True


def upgrade_client_judge(data, nonce, max_response=0):
    """One client connection's first bytes as WSClient::onReceived,
    HTTPResponse::Parse and WebSocket::PerformClientUpgrade judge them against
    the 16-byte ``nonce``.  Returns a dict: code, status, consumed, need,
    accept (offset, length) or None, body (offset, length) or None, and fail:
    the code of the header that ended the walk (0: none), which the classes
    report through onWSError even where the outcome is UC_ACCEPTED."""
    data = bytes(data)
    out = dict(code=UC_TOO_LONG if max_response and len(data) >= max_response else UC_INCOMPLETE, status=0, consumed=0,
               need=0, accept=None, body=None, fail=0)
    p = data.find(b"\r\n\r\n")
    if p < 0:
        return out
    hend = p + 4
    eol = data.find(b"\r\n")
    line = data[:eol]
    s1 = line.find(b" ")
    s2 = line.find(b" ", s1 + 1) if s1 >= 0 else -1
    digits = line[s1 + 1:s2 if s2 >= 0 else len(line)]
    bad = s1 <= 0 or len(digits) != 3 or not all(48 <= c <= 57 for c in digits)
    headers, clen, at = [], 0, eol + 2
    block_end = max(hend - 2, at)
    while not bad and at < block_end:
        e = data.find(b"\r\n", at, block_end)
        e = block_end if e < 0 else e
        ln = data[at:e]
        if ln:
            colon = ln.find(b":")
            if colon <= 0:
                bad = True
                break
            k, v = ln[:colon].strip(b" \t"), ln[colon + 1:].strip(b" \t")
            v_at = at + colon + 1 + (len(ln[colon + 1:]) - len(ln[colon + 1:].lstrip(b" \t")))
            headers.append((_lower(k), v, v_at))
            if _lower(k) == b"content-length":
                clen = 0
                for c in v:
                    if not 48 <= c <= 57:
                        bad = True
                        break
                    clen = (clen * 10 + c - 48) % 2**64
        at = e + 2
    if bad:
        out.update(code=UC_BAD_HTTP, consumed=hend)
        return out
    if len(data) - hend < clen:
        out["need"] = min(hend + clen, U64_MAX)
        return out
    status = int(digits)
    out.update(code=UC_NOT_101, status=status, consumed=hend + clen, body=(hend, min(clen, 0xFFFFFFFF)))
    if status != 101:
        return out
    expect = upgrade_expect(nonce)
    seen, fail = set(), 0
    for k, v, v_at in headers:
        if k == b"connection":
            if _lower(v) != b"upgrade":
                fail = UC_BAD_CONNECTION
        elif k == b"upgrade":
            if _lower(v) != b"websocket":
                fail = UC_BAD_UPGRADE
        elif k == b"sec-websocket-accept":
            out["accept"] = (v_at, min(len(v), 0xFFFFFFFF))
            if not _accept_ok(v, expect):
                fail = UC_BAD_ACCEPT
        else:
            continue
        if fail:
            break
        seen.add(k)
    out.update(code=UC_ACCEPTED if len(seen) == 3 else fail or UC_MISSING, fail=fail)
    return out


def upgrade_client_plan(wire, spans, nonces, max_response=0):
    """wsg_upgrade_client_streams restated on the host: one response per
    stream ``wire[off, off + len)`` against ``nonces[16 j, 16 j + 16)``.
    Returns (up, consumed, need, count, bad): UPGRADE_REPLY_DTYPE records, the
    spans' outputs, count = [accepted, whole but not accepted, incomplete] and
    the spans latched as WSG_EINVAL (bad_spans)."""
    wire = np.asarray(wire, dtype=np.uint8)
    spans = np.asarray(spans, dtype=STREAM_SPAN)
    nonces = np.asarray(nonces, dtype=np.uint8).reshape(-1)
    ns = len(spans)
    assert len(nonces) == 16 * ns
    bad = bad_spans(len(wire), spans)
    up = np.zeros(ns, dtype=UPGRADE_REPLY_DTYPE)
    consumed = np.zeros(ns, dtype=np.uint64)
    need = np.zeros(ns, dtype=np.uint64)
    for j in range(ns):
        if bad[j]:
            continue
        off, length = int(spans["off"][j]), int(spans["len"][j])
        o = upgrade_client_judge(wire[off:off + length].tobytes(), nonces[16 * j:16 * j + 16].tobytes(), max_response)
        u = up[j]
        u["code"], u["status"] = o["code"], o["status"]
        if o["accept"] is not None:
            u["accept_off"], u["accept_len"] = off + o["accept"][0], o["accept"][1]
        if o["body"] is not None:
            u["body_off"], u["body_len"] = off + o["body"][0], o["body"][1]
        consumed[j], need[j] = o["consumed"], o["need"]
    code = up["code"]
    count = np.array([np.sum(code == UC_ACCEPTED), np.sum((code >= UC_BAD_HTTP) & (code <= UC_NOT_101)),
                      np.sum(code == UC_INCOMPLETE)], dtype=np.uint64)
    return up, consumed, need, count, bad


# wsg_stream_read: where a stream's new bytes lie in a wsg_carry_streams call's d_new.
STREAM_READ = np.dtype([("off", "<u8"), ("len", "<u8")])

assert STREAM_READ.itemsize == 16


def carry_plan(wire, spans, new, reads, close_off=None, next_cap=None):
    """wsg_carry_streams restated on the host, from its contract: the next
    round's wire is, per stream, the tail ``wire[off + consumed, off + len)``
    followed by the read ``new[read.off, read.off + read.len)``.

    ``spans``: STREAM_SPAN records as the last round's calls left them;
    ``reads``: STREAM_READ records or None (no stream has new bytes);
    ``close_off``: None, or per stream a word that drops the stream unless it
    is 2**64 - 1.  Returns (next, next_spans, count, key): the bytes of
    d_next[0, count[0]), every stream at the next multiple of 16 behind the
    one before it and the padding zero; the STREAM_SPAN records {off, len,
    0, 0}; count = [bytes of next, tail bytes, new bytes, streams dropped];
    and the latch's key, None when nothing is latched: the smallest of
    stream << 8 | 22 over the streams refused (a span bad_spans refuses,
    consumed > len, or, on a stream not dropped, a read past the end of
    ``new``; such a stream is empty) and, given ``next_cap``, n_streams << 8
    | 12 when count[0] exceeds it (the call then writes no byte of d_next)."""
    wire = np.asarray(wire, dtype=np.uint8)
    new = np.asarray(new, dtype=np.uint8)
    spans = np.asarray(spans, dtype=STREAM_SPAN)
    ns = len(spans)
    bad = bad_spans(len(wire), spans)
    out = np.zeros(ns, dtype=STREAM_SPAN)
    parts, at, tails, news, dropped, key = [], 0, 0, 0, 0, None
    for j in range(ns):
        off, length, used = (int(spans[f][j]) for f in ("off", "len", "consumed"))
        drop = close_off is not None and int(close_off[j]) != U64_MAX
        dropped += drop
        refused = bool(bad[j]) or used > length
        tail = fresh = b""
        if not refused and not drop:
            tail = wire[off + used: off + length].tobytes()
            if reads is not None:
                r_off, r_len = int(reads["off"][j]), int(reads["len"][j])
                if r_off + r_len > len(new):
                    refused = True
                else:
                    fresh = new[r_off: r_off + r_len].tobytes()
        if refused:
            tail = fresh = b""
            if key is None:
                key = j << 8 | -WSG_EINVAL
        size = len(tail) + len(fresh)
        out["off"][j], out["len"][j] = at, size
        parts += [tail, fresh, bytes(-size % 16)]
        at += size + -size % 16
        tails += len(tail)
        news += len(fresh)
    if key is None and next_cap is not None and at > next_cap:
        key = ns << 8 | -WSG_ENOMEM
    count = np.array([at, tails, news, dropped], dtype=np.uint64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), out, count, key
