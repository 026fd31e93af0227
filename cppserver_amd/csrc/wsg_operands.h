// wsg_operands.h — the operands of the device entry points that always travel
// together, named once.  An entry point of wsg_capi_device.cpp fills them from
// its parameters, wsg_args.h reads its argument checks off them, and the host
// launchers (wsg_internal.h) take them by const reference and unpack them at
// the <<<>>> call: no kernel sees a group.  Plain aggregates, no HIP.
#pragma once

#include <stdint.h>

#include "wsg_capi.h"

namespace wsg {

// A batch of frames: the wire, the frame table, the streams' first frames.
// (d_state travels beside it: read by some calls, written by others.)
struct Batch {
    const uint8_t* wire;
    uint64_t wire_len;
    const uint64_t* fs;             // n frame starts
    uint32_t n;
    const uint32_t* stream_first;   // n_streams + 1
    uint32_t n_streams;
};

// What the message plan writes for its caller.
struct MsgOut {
    wsg_msg* msgs;
    uint64_t* count;
    wsg_recv_info* info;
};

// The caller's rule, by value in the kernels' arguments.
struct ReplyRule {
    uint8_t op[5];   // by WSG_CB_*: the reply's first header byte, 0 (none) or WSG_REPLY_SAME
    uint8_t mask;
};
inline ReplyRule reply_rule(const uint8_t op[5], int mask)
{
    return ReplyRule{{op[0], op[1], op[2], op[3], op[4]}, uint8_t(mask ? 1 : 0)};
}

// The reply side of wsg_reply_messages and of the checked replies.
struct ReplyOut {
    const uint8_t* reply_op;    // 5, the caller's (host memory)
    int mask;
    const uint32_t* send_key;   // n_streams, or null
    uint8_t* reply;
    uint64_t reply_cap;
    uint64_t* reply_off;        // n + 1
    uint64_t* stream_reply;     // n_streams + 1
    uint64_t* close_off;        // n_streams; null: wsg_reply_messages, which closes nothing
};

// The protocol check's operands (wsg_check_protocol, the checked replies).
struct ProtoOps {
    wsg_proto_state* proto;
    uint32_t role;
    uint64_t max_message;
    const wsg_proto_verdict* also;   // or null
    wsg_proto_verdict* verdict;
    uint64_t* result;                // 3 words
};

// What wsg_reply_validated adds to the checked reply: the UTF-8 check from the
// wire between the protocol judge and the merge, on the dense piece records of
// k_msg_finalize, and its verdicts merged with the caller's.
struct Utf8Inside {
    uint32_t which;
    uint64_t* valid;     // n words
    uint64_t* result;    // 4 words
    uint64_t* also;      // n_streams words of scratch: the merged d_also
    int rec_grid;        // blocks of the per-record kernels (at least one)
    int wire_grid;       // blocks of k_utf8_wire
};

// What wsg_relay_validated adds to wsg_reply_validated's arguments.
struct RelayArgs {
    const uint8_t* relay_op;       // 5, the caller's (host memory)
    const uint32_t* order;         // n_streams, or null
    const uint32_t* group_first;   // n_groups + 1, or null (one group)
    uint32_t n_groups;
    uint8_t* relay;
    uint64_t relay_cap;
    uint64_t* relay_off;           // n
    uint64_t* group_relay;         // n_groups + 1
};

// What a _streams form has in the place of a frame table: the framer's
// operands.  Its Batch holds frame_start, frame_cap and stream_first as fs, n
// and stream_first until the frame count is known.
struct Framed {
    wsg_stream_span* span;      // n_streams
    uint64_t* frame_start;      // frame_cap
    uint32_t frame_cap;
    uint32_t* stream_first;     // n_streams + 1
    uint32_t* n_frames_out;     // the caller's (host memory)
};

} // namespace wsg
