// wsg_args.h — the argument checks of the device entry points of
// include/wsg_capi.h, one table per family.  An operand is a row: pointer,
// bytes, alignment and whether it may be null; args_check walks the rows.
// What an entry point accepts is its args_* function below and nothing else:
// the rows, and beside them the few conditions that are not one operand's.
// Host only and without HIP: tests/cpp/test_capi_args.cpp runs every one of
// them without a device.
//
// The rules differ by entry point and are part of the contract of wsg_capi.h:
// the older entry points test the alignment of their 16-byte operands alone,
// the later ones of every operand (`a8` below: 1 or 8), and an entry point
// checks the words of d_count and d_result it writes.
#pragma once

#include <cstdint>
#include <initializer_list>

#include "wsg_capi.h"
#include "wsg_operands.h"

// [p, p + bytes) lies in one device allocation (wsg_capi.cpp; $WSG_CHECK=1).
bool in_alloc(const void* p, uint64_t bytes);

namespace wsg {

enum ArgKind : uint8_t {
    ARG_ALWAYS,     // never null
    ARG_SIZED,      // null only when bytes == 0
    ARG_OPTIONAL,   // null: not given
};

struct ArgRow {
    const void* p;
    uint64_t bytes;    // what the kernels may touch from p on
    uint32_t align;    // 1, 4, 8 or 16
    ArgKind kind;
};

inline ArgRow always(const void* p, uint64_t bytes, uint32_t align) { return {p, bytes, align, ARG_ALWAYS}; }
inline ArgRow sized(const void* p, uint64_t bytes, uint32_t align) { return {p, bytes, align, ARG_SIZED}; }
inline ArgRow optional(const void* p, uint64_t bytes, uint32_t align) { return {p, bytes, align, ARG_OPTIONAL}; }
// Required by a count that is not the row's bytes.
inline ArgRow when(bool required, const void* p, uint64_t bytes, uint32_t align)
{
    return {p, bytes, align, required ? ARG_ALWAYS : ARG_OPTIONAL};
}
// A wire the kernels read in 16-byte chunks: 16-byte aligned, the allocation
// holds the last chunk whole.  (Required by len, not by the rounded count,
// which wraps to 0 for a len within 15 of 2^64.)
inline ArgRow wire(const void* p, uint64_t len) { return when(len != 0, p, (len + 15) & ~uint64_t(15), 16); }
// The place of a row that a variant of the family does not have.
inline ArgRow absent() { return optional(nullptr, 0, 1); }

// WSG_EINVAL for a null row that may not be, a misaligned row and, under
// `check`, a row given whose bytes in_alloc refuses.
inline int args_check(std::initializer_list<ArgRow> rows, bool check)
{
    for (const ArgRow& r : rows) {
        if (!r.p) {
            if (r.kind == ARG_ALWAYS || (r.kind == ARG_SIZED && r.bytes))
                return WSG_EINVAL;
        } else if (reinterpret_cast<uintptr_t>(r.p) & (r.align - 1)) {
            return WSG_EINVAL;
        }
    }
    if (check)
        for (const ArgRow& r : rows)
            if (r.p && !in_alloc(r.p, r.bytes))
                return WSG_EINVAL;
    return WSG_OK;
}

inline int args_decode_batch(const void* d_wire, uint64_t wire_len, const void* fs, uint32_t n, const void* out,
                             const void* info, bool check)
{
    return args_check({wire(d_wire, wire_len), sized(out, wire_len, 16), sized(fs, uint64_t(n) * 8, 1),
                       sized(info, uint64_t(n) * sizeof(wsg_recv_info), 1)},
                      check);
}

// The message plan's family.  Decodes: wsg_decode_messages (r null, msg and
// msg_cap) and wsg_check_utf8_wire (u: valid and 4 words of result; every
// operand aligned).  Replies (r): wsg_reply_messages (p null: no close_off, 4
// words of d_count, 16-byte operands alone aligned); wsg_reply_checked (p; 5
// words), with u wsg_reply_validated, with q too wsg_relay_validated (8
// words).  f: the _streams form of any, whose b.n is a capacity: any value,
// and one above 0 with no stream is not refused (it finds no frame); d_span
// and n_frames_out besides.
inline int args_messages(const Batch& b, const void* state, const void* msg, uint64_t msg_cap, const ReplyOut* r,
                         const MsgOut& o, const ProtoOps* p, const Utf8Inside* u, const RelayArgs* q, const Framed* f,
                         bool check)
{
    if (b.n_streams == UINT32_MAX || (!f && (b.n == UINT32_MAX || (b.n && b.n_streams == 0))) ||
        (f && !f->n_frames_out) || (r && !r->reply_op) || (p && p->role > WSG_PROTO_CLIENT))
        return WSG_EINVAL;
    if (q) {
        if (!q->relay_op || (!q->group_first && q->n_groups != 1) || (q->n_groups == 0 && b.n_streams != 0) ||
            q->n_groups == UINT32_MAX)
            return WSG_EINVAL;
        for (int k = 0; k < 5; ++k)
            if (q->relay_op[k] && r->reply_op[k])
                return WSG_EINVAL;   // a kind is replied to or relayed, not both
    }
    const uint32_t a8 = (p || (u && !r)) ? 8 : 1, a4 = a8 == 8 ? 4 : 1;
    const uint64_t n = b.n, ns = b.n_streams, ng = q ? q->n_groups : 0;
    return args_check(
        {wire(b.wire, b.wire_len),
         sized(b.fs, n * 8, a8),
         always(b.stream_first, (ns + 1) * 4, a4),
         sized(state, ns * sizeof(wsg_stream_state), a8),
         sized(o.msgs, n * sizeof(wsg_msg), a8),
         always(o.count, (q ? 8 : p ? 5 : r ? 4 : 2) * 8, a8),
         sized(o.info, n * sizeof(wsg_recv_info), a8),
         f ? sized(f->span, ns * sizeof(wsg_stream_span), 1) : absent(),
         sized(msg, msg_cap, 16),
         r ? optional(r->send_key, ns * 4, a4) : absent(),
         r ? sized(r->reply, r->reply_cap, 16) : absent(),
         r ? always(r->reply_off, (n + 1) * 8, a8) : absent(),
         r ? always(r->stream_reply, (ns + 1) * 8, a8) : absent(),
         p ? always(r->close_off, ns * 8, 8) : absent(),
         p ? always(p->proto, ns * sizeof(wsg_proto_state), 8) : absent(),
         p ? optional(p->also, ns * sizeof(wsg_proto_verdict), 8) : absent(),
         p ? always(p->verdict, ns * sizeof(wsg_proto_verdict), 8) : absent(),
         p ? always(p->result, 3 * 8, 8) : absent(),
         u ? sized(u->valid, n * 8, 8) : absent(),
         u ? always(u->result, 4 * 8, 8) : absent(),
         q ? optional(q->order, ns * 4, 4) : absent(),
         q ? optional(q->group_first, (ng + 1) * 4, 4) : absent(),
         q ? sized(q->relay, q->relay_cap, 16) : absent(),
         q ? sized(q->relay_off, n * 8, 8) : absent(),
         q ? always(q->group_relay, (ng + 1) * 8, 8) : absent()},
        check);
}

inline int args_check_utf8(const void* msg, uint64_t msg_cap, const void* msgs, const void* count, uint32_t msg_room,
                           const void* valid, const void* result, bool check)
{
    return args_check({sized(msg, msg_cap, 16), sized(msgs, uint64_t(msg_room) * sizeof(wsg_msg), 8),
                       sized(valid, uint64_t(msg_room) * 8, 8), always(count, 2 * 8, 8), always(result, 4 * 8, 8)},
                      check);
}

// wsg_check_protocol (b.fs unused).  Its outputs are required for no frame and
// no stream too, d_state is optional, and the wire is read by the byte:
// neither rounded nor aligned.
inline int args_check_protocol(const Batch& b, const void* info, const void* state, const ProtoOps& p, bool check)
{
    if (p.role > WSG_PROTO_CLIENT || b.n == UINT32_MAX || b.n_streams == UINT32_MAX)
        return WSG_EINVAL;
    const uint64_t ns = b.n_streams;
    return args_check({sized(b.wire, b.wire_len, 1), always(info, uint64_t(b.n) * sizeof(wsg_recv_info), 8),
                       always(b.stream_first, (ns + 1) * 4, 4), optional(state, ns * sizeof(wsg_stream_state), 8),
                       always(p.proto, ns * sizeof(wsg_proto_state), 8),
                       always(p.verdict, ns * sizeof(wsg_proto_verdict), 8), always(p.result, 3 * 8, 8)},
                      check);
}

inline int args_frame_streams(const void* d_wire, uint64_t wire_len, const void* span, uint32_t n_streams,
                              const void* frame_start, uint32_t frame_cap, const void* stream_first, const void* count,
                              bool check)
{
    if (n_streams == UINT32_MAX)
        return WSG_EINVAL;
    return args_check({wire(d_wire, wire_len), sized(span, uint64_t(n_streams) * sizeof(wsg_stream_span), 1),
                       sized(frame_start, uint64_t(frame_cap) * 8, 1),
                       always(stream_first, (uint64_t(n_streams) + 1) * 4, 1), always(count, 2 * 8, 1)},
                      check);
}

inline int args_upgrade_streams(const void* d_wire, uint64_t wire_len, const void* span, uint32_t n_streams,
                                const void* up, const void* resp, uint64_t resp_cap, const void* resp_off,
                                const void* count, bool check)
{
    if (n_streams == UINT32_MAX)
        return WSG_EINVAL;
    return args_check({wire(d_wire, wire_len), sized(span, uint64_t(n_streams) * sizeof(wsg_stream_span), 8),
                       sized(up, uint64_t(n_streams) * sizeof(wsg_upgrade), 8), sized(resp, resp_cap, 16),
                       always(resp_off, (uint64_t(n_streams) + 1) * 8, 8), always(count, 4 * 8, 8)},
                      check);
}

inline int args_upgrade_client(const void* d_wire, uint64_t wire_len, const void* span, uint32_t n_streams,
                               const void* nonce, const void* up, const void* count, bool check)
{
    if (n_streams == UINT32_MAX)
        return WSG_EINVAL;
    const uint64_t ns = n_streams;
    return args_check({wire(d_wire, wire_len), sized(span, ns * sizeof(wsg_stream_span), 8), sized(nonce, ns * 16, 16),
                       sized(up, ns * sizeof(wsg_upgrade_reply), 8), always(count, 3 * 8, 8)},
                      check);
}

// wsg_upgrade_requests; total = n * tpl_len, which the entry point has held
// against req_cap (WSG_ENOMEM) when it asks.  The template is read in 16-byte
// blocks; nothing is needed for no request.
inline int args_upgrade_requests(const void* tpl, uint32_t tpl_len, uint32_t key_at, const void* nonce, uint32_t n,
                                 const void* req, uint64_t total, bool check)
{
    if (uint64_t(key_at) + 24 > tpl_len)
        return WSG_EINVAL;
    return args_check({when(n != 0, tpl, (uint64_t(tpl_len) + 15) & ~uint64_t(15), 16),
                       sized(nonce, uint64_t(n) * 16, 16), when(n != 0, req, total, 16)},
                      check && n != 0);
}

// wsg_carry_streams: the next wire overlaps neither source, the next spans are
// not the spans.
inline int args_carry_streams(const uint8_t* d_wire, uint64_t wire_len, const void* span, uint32_t n_streams,
                              const void* close_off, const uint8_t* fresh, uint64_t new_len, const void* read,
                              const uint8_t* next, uint64_t next_cap, const void* next_span, const void* count,
                              bool check)
{
    const auto overlap = [](const uint8_t* a, uint64_t an, const uint8_t* b, uint64_t bn) {
        return an && bn && a < b + bn && b < a + an;
    };
    if (n_streams == UINT32_MAX || (n_streams && next_span == span) || overlap(next, next_cap, d_wire, wire_len) ||
        overlap(next, next_cap, fresh, new_len))
        return WSG_EINVAL;
    const uint64_t ns = n_streams;
    return args_check({wire(d_wire, wire_len), wire(fresh, new_len), sized(next, next_cap, 16),
                       sized(span, ns * sizeof(wsg_stream_span), 8), optional(close_off, ns * 8, 8),
                       optional(read, ns * sizeof(wsg_stream_read), 8),
                       sized(next_span, ns * sizeof(wsg_stream_span), 8), always(count, 4 * 8, 8)},
                      check);
}

inline int args_utf8_verdicts(const void* msgs, const void* count, uint32_t msg_room, const void* valid,
                              uint32_t n_streams, const void* also, bool check)
{
    if (n_streams == UINT32_MAX)
        return WSG_EINVAL;
    return args_check({sized(msgs, uint64_t(msg_room) * sizeof(wsg_msg), 8), sized(valid, uint64_t(msg_room) * 8, 8),
                       always(count, 2 * 8, 8), sized(also, uint64_t(n_streams) * sizeof(wsg_proto_verdict), 8)},
                      check);
}

// wsg_encode_batch: nothing but the one word of d_wire_off is touched for no
// frame, so nothing is looked up then.  (The payload ranges are the
// descriptors', which the entry point reads back under WSG_CHECK.)
inline int args_encode_batch(const void* desc, uint32_t n, const void* d_wire, uint64_t wire_cap, const void* wire_off,
                             bool check)
{
    return args_check({sized(desc, uint64_t(n) * sizeof(wsg_send_desc), 1), when(n != 0, d_wire, wire_cap, 16),
                       always(wire_off, (uint64_t(n) + 1) * 8, 1)},
                      check && n != 0);
}

// wsg_fanout_encode; total: the bytes of its k frames.  The entry point asks
// twice: without `check` first, and under it once k == 0 and total > wire_cap
// (WSG_ENOMEM) have had their turn.
inline int args_fanout_encode(const void* payload, uint64_t len, const void* keys, uint32_t k, const void* d_wire,
                              uint64_t total, bool check)
{
    return args_check({sized(payload, len, 1), sized(keys, uint64_t(k) * 4, 1), when(k != 0, d_wire, total, 16)}, check);
}

// wsg_fanout_encode_many, twice in the same way (total 0 the first time: the
// sizes are read from tables this refuses when null).  The messages' payload
// ranges stay with the entry point.
inline int args_fanout_encode_many(const void* src_off, const void* len, const void* opcode, uint32_t m,
                                   const void* keys, uint32_t k, const void* d_wire, uint64_t total,
                                   const void* wire_off, bool check)
{
    if (!wire_off || (m && (!src_off || !len || !opcode)))   // (host memory)
        return WSG_EINVAL;
    return args_check({when(m && k, keys, uint64_t(k) * 4, 1), when(m && k, d_wire, total, 16)}, check);
}

} // namespace wsg
