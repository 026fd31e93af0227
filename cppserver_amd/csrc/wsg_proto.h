// wsg_proto.h — the frame-sequence rules of RFC 6455 (5.1, 5.2, 5.4, 5.5, 7.4)
// as one transition and one judgement per frame, shared by the host helper
// wsg_proto_judge and the gfx950 kernels of wsg_check_protocol (one source of
// truth, as wsg_frame.h is for the frame arithmetic and wsg_utf8.h for UTF-8).
//
// The reference accepts RSV bits, reserved opcodes, unmasked client frames,
// fragmented or long control frames, stray continuations, interleaved data
// frames and malformed close frames silently; an endpoint must fail such a
// connection with status 1002, and with 1009 a message that outgrows its limit.
//
// A stream's state before a frame is (open, bytes): a data message has begun
// and not had its FIN frame, and the payload bytes of that message so far.
// The transition (proto_step, applied with proto_then) is total: it applies
// whether or not the frame violates a rule.  proto_code is the
// lowest-numbered WSG_PV_* that applies to the frame.
#pragma once

#include <stdint.h>

#include "wsg_frame.h"

namespace wsg {

// What the rule reads of a wsg_recv_info record.
struct ProtoFrame {
    uint64_t payload_off;
    uint64_t len;
    uint32_t key;
    uint32_t op;       // opcode field (b0 & 0x0F)
    uint32_t rsv;      // b0 & 0x70
    bool fin, masked, error;
};

// From the record's four 8-byte words (the kernels load it that way).
WSG_HD ProtoFrame proto_frame(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3)
{
    ProtoFrame f;
    f.payload_off = w0;
    f.len = w1;
    f.key = uint32_t(w2);
    f.op = uint32_t(w2 >> 32) & 0xFFu;
    f.fin = ((w2 >> 40) & 0xFFu) != 0;
    f.masked = ((w2 >> 48) & 0xFFu) != 0;
    f.rsv = uint32_t(w3) & 0x70u;
    f.error = ((w3 >> 8) & 0xFFu) != 0;
    return f;
}

WSG_HD bool proto_control(uint32_t op) { return (op & 8u) != 0; }
WSG_HD bool proto_reserved(uint32_t op) { return (op >= 3u && op <= 7u) || op >= 0xBu; }

WSG_HD uint64_t proto_sat_add(uint64_t a, uint64_t b) { return a + b < a ? UINT64_MAX : a + b; }

// The transition as an element of a scan: keep the state, add len and set
// open, or set (len, open).  Composition (proto_then) is associative because
// the saturating sum is.
enum : uint32_t { PROTO_KEEP = 0, PROTO_ADD = 1, PROTO_SET = 2 };
struct ProtoStep {
    uint64_t bytes;
    uint32_t kind;   // PROTO_*
    uint32_t open;   // 0 / 1 (ADD and SET)
};

WSG_HD ProtoStep proto_step(const ProtoFrame& f)
{
    if (f.error || f.op > 2u)   // control, reserved or not a frame: unchanged
        return ProtoStep{0, PROTO_KEEP, 0};
    return ProtoStep{f.len, f.op == 0u ? uint32_t(PROTO_ADD) : uint32_t(PROTO_SET), f.fin ? 0u : 1u};
}

// a, then b
// (operands by value and the result field by field: a choice between two
// structs by reference became a choice between their addresses, and the block
// scan's running value then lived in scratch memory)
WSG_HD ProtoStep proto_then(ProtoStep a, ProtoStep b)
{
    const uint64_t ab = a.bytes, bb = b.bytes;
    const uint32_t ak = a.kind, bk = b.kind, ao = a.open, bo = b.open;
    const bool keep_a = bk == PROTO_KEEP;
    const bool take_b = bk == PROTO_SET || ak == PROTO_KEEP;
    ProtoStep r;
    r.bytes = keep_a ? ab : take_b ? bb : proto_sat_add(ab, bb);   // else b adds to a
    r.kind = keep_a || !take_b ? ak : bk;
    r.open = keep_a ? ao : bo;
    return r;
}

// A state as the step that sets it: proto_then(proto_seed(s), step) is the
// state the step leaves behind s (always a "set").
WSG_HD ProtoStep proto_seed(uint64_t bytes, bool open) { return ProtoStep{bytes, PROTO_SET, open ? 1u : 0u}; }

WSG_HD bool proto_status_ok(uint32_t s)
{
    return (s >= 1000u && s <= 1003u) || (s >= 1007u && s <= 1014u) || (s >= 3000u && s <= 4999u);
}

// The judgement of frame f whose stream was (open, bytes) before it and holds
// bytes_after behind it: the code (0: none) and the close status that goes
// with it.  wire_status() reads the status a close frame carries (asked only
// for an op 8 frame with len >= 2 that no lower rule stops).
template <class WireStatus>
WSG_HD uint32_t proto_code(const ProtoFrame& f, bool open, uint64_t bytes_after, uint32_t role, uint64_t max_message,
                           WireStatus wire_status, uint32_t* status)
{
    *status = 1002;
    if (f.error)
        return WSG_PV_FRAME;
    if (f.rsv)
        return WSG_PV_RSV;
    if (proto_reserved(f.op))
        return WSG_PV_OPCODE;
    if ((role == WSG_PROTO_SERVER && !f.masked) || (role == WSG_PROTO_CLIENT && f.masked))
        return WSG_PV_MASK;
    if (proto_control(f.op)) {
        if (!f.fin)
            return WSG_PV_CTRL_FRAGMENT;
        if (f.len > 125)
            return WSG_PV_CTRL_LONG;
        if (f.op != WSG_CLOSE) {
            *status = 0;
            return 0;
        }
        if (f.len == 1)
            return WSG_PV_CLOSE_LEN;
        uint32_t carried = 1005;
        if (f.len >= 2) {
            carried = wire_status();
            if (!proto_status_ok(carried))
                return WSG_PV_CLOSE_CODE;
        }
        *status = carried;
        return WSG_PV_CLOSED;
    }
    if (f.op == 0u && !open)
        return WSG_PV_CONT;
    if (f.op != 0u && open)
        return WSG_PV_DATA;
    if (max_message != 0 && bytes_after > max_message) {
        *status = 1009;
        return WSG_PV_TOO_BIG;
    }
    *status = 0;
    return 0;
}

// The two status bytes at the head of a close payload, unmasked, big-endian.
WSG_HD uint32_t proto_wire_status(uint32_t b0, uint32_t b1, const ProtoFrame& f)
{
    if (f.masked) {
        b0 ^= key_byte(f.key, 0);
        b1 ^= key_byte(f.key, 1);
    }
    return ((b0 & 0xFFu) << 8) | (b1 & 0xFFu);
}

// wsg_proto_verdict as one little-endian word: it orders by frame first.
WSG_HD uint64_t proto_verdict_word(uint32_t code, uint32_t status, uint32_t frame)
{
    return uint64_t(code & 0xFFu) | (uint64_t(status & 0xFFFFu) << 16) | (uint64_t(frame) << 32);
}

} // namespace wsg
