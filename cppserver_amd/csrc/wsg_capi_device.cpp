// wsg_capi_device.cpp — the device-resident entry points of include/wsg_capi.h
// (wsg_decode_batch through wsg_relay_validated_streams, wsg_utf8_verdicts,
// wsg_encode_batch and the fan-outs): scratch and launches.  An entry point
// fills the operand groups of wsg_operands.h from its parameters once; what it
// accepts is its args_* function of wsg_args.h.  Operands are device memory;
// nothing here synchronises but wsg_*_streams, which read a frame count back.
#include "wsg_ctx.h"

#include <vector>

int decode_launch(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start, uint32_t n,
                  uint8_t* d_out, wsg_recv_info* d_info, hipStream_t s, unsigned long long* err)
{
    if (n == 0) {
        if (wire_len && d_out != d_wire)
            WSG_HIP(hipMemcpyAsync(d_out, d_wire, wire_len, hipMemcpyDeviceToDevice, s));
        return WSG_OK;
    }
    // every tile, and at least one block per 256 frames so that the frames of
    // a short (or empty) wire are still checked
    const uint64_t tiles = ceil_div(wire_len, wsg::TILE);
    const int t = timing_begin(c, s);
    WSG_HIP(wsg::launch_decode(s, grid_for(c, std::max(tiles, ceil_div(n, wsg::BLOCK)), c->dec_blocks_per_cu), d_wire, d_out, wire_len,
                               d_frame_start, n, d_info, err));
    timing_end(c, s, t);
    return WSG_OK;
}

namespace {

// upper bound of the pieces: sum of ceil((size + 15) / PIECE) over frames
inline uint64_t pieces_bound(uint32_t n, uint64_t wire_cap) { return wire_cap / wsg::PIECE + 2 * uint64_t(n) + 1; }

// A wave per piece, under the caller's cap: the grid of the gathers, of
// k_utf8_wire, of k_encode_mask and of the carry's copy.
int piece_grid(const wsg_ctx* c, uint64_t pieces, int blocks_per_cu)
{
    return grid_for(c, ceil_div(pieces, wsg::BLOCK / 64), blocks_per_cu);
}

// The scratch of wsg_decode_messages / wsg_reply_messages for n frames of a
// wire of wire_len bytes: the plan block and the piece records.  Pieces: at
// most len / PIECE + 2 per delivered frame, and the delivered payloads of a
// well-formed batch are disjoint ranges of the wire (the kernels clamp to
// this bound whatever the batch holds); a reply cuts the same frames at
// 16-byte chunks of another destination.  Both are the context's: entered
// behind the previous call's kernels, whatever stream they ran on.
// Under WSG_ASSEMBLY_RFC the plan block holds that rule's scans behind the
// reference rule's (which its reply kernels and the gather share).
int msg_scratch(wsg_ctx* c, hipStream_t s, uint32_t n, uint64_t wire_len, wsg::MsgScratch* x, bool* ordered)
{
    x->pieces_cap = pieces_bound(n, wire_len);
    if (x->pieces_cap > UINT32_MAX)
        return WSG_EINVAL;
    x->plans.assembly = c->assembly;
    const bool rfc = c->assembly == WSG_ASSEMBLY_RFC;
    const uint64_t ref_bytes = (wsg::msg_plan_layout(nullptr, n, nullptr) + 15) & ~uint64_t(15);
    if (int rc = ensure_array(c->d_msg_plan, c->msg_plan_cap,
                              ref_bytes + (rfc ? wsg::rfc_plan_layout(nullptr, n, nullptr) : 0)))
        return rc;
    if (int rc = ensure_array(c->d_msg_pieces, c->msg_pieces_cap, x->pieces_cap))
        return rc;
    wsg::msg_plan_layout(c->d_msg_plan, n, &x->plans.ref);
    x->plans.rfc = wsg::RfcPlan{};
    if (rfc)
        wsg::rfc_plan_layout(c->d_msg_plan + ref_bytes, n, &x->plans.rfc);
    x->pieces = c->d_msg_pieces;
    x->err = c->d_err;
    return scratch_enter(c->msg_order, s, ordered);
}

// The scratch of wsg_check_protocol / wsg_reply_checked for n frames in
// n_streams streams: the plan block, the context's, entered as msg_scratch's.
// `also` (wsg_reply_validated): n_streams more words behind that block, the
// merged verdicts its reply kernels read, under the same order.
int proto_scratch(wsg_ctx* c, hipStream_t s, uint32_t n, uint32_t n_streams, wsg::ProtoPlan* plan, bool* ordered,
                  uint64_t** also = nullptr)
{
    const uint64_t block = (wsg::proto_plan_layout(nullptr, n, n_streams, nullptr) + 15) & ~uint64_t(15);
    if (int rc = ensure_array(c->d_proto_plan, c->proto_plan_cap, block + (also ? uint64_t(n_streams) * 8 : 0)))
        return rc;
    wsg::proto_plan_layout(c->d_proto_plan, n, n_streams, plan);
    if (also)
        *also = reinterpret_cast<uint64_t*>(c->d_proto_plan + block);
    return scratch_enter(c->proto_order, s, ordered);
}

// The gather over piece records, the timed kernel of its call; tot: which
// pieces (wsg::launch_gather).
int gather_launch(wsg_ctx* c, hipStream_t s, const uint8_t* d_wire, const uint64_t* tot, const wsg::MsgScratch& x,
                  uint8_t* d_dst, uint64_t dst_cap)
{
    const int t = timing_begin(c, s);
    WSG_HIP(wsg::launch_gather(s, piece_grid(c, x.pieces_cap, c->enc_blocks_per_cu), d_wire, tot, x.pieces,
                               x.pieces_cap, d_dst, dst_cap));
    timing_end(c, s, t);
    return WSG_OK;
}

// wsg_relay_validated's scratch for n frames in n_streams streams: the plan
// block and piece records of its own (the reply's gather reads the message
// plan's while the relay's are written), the context's, under the message
// plan's order, which the caller has entered.
int relay_scratch(wsg_ctx* c, uint32_t n, uint32_t n_streams, uint64_t pieces_cap, wsg::RelayPlan* plan)
{
    const uint64_t block = wsg::relay_plan_layout(nullptr, n, n_streams, nullptr);
    if (int rc = ensure_array(c->d_relay_plan, c->relay_plan_cap, block))
        return rc;
    if (int rc = ensure_array(c->d_relay_pieces, c->relay_pieces_cap, pieces_cap))
        return rc;
    wsg::relay_plan_layout(c->d_relay_plan, n, n_streams, plan);
    return WSG_OK;
}

} // namespace

int wsg_decode_batch(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start, uint32_t n,
                     uint8_t* d_out, wsg_recv_info* d_info, void* stream)
{
    if (!c || wsg::args_decode_batch(d_wire, wire_len, d_frame_start, n, d_out, d_info, c->check))
        return WSG_EINVAL;
    return decode_launch(c, d_wire, wire_len, d_frame_start, n, d_out, d_info, as_stream(stream), c->d_err);
}

namespace {

// Messages out of a batch of frames: the plan pass (a few small kernels, one
// lane per frame or per stream), then the gather, which moves every
// delivered payload byte once, to d_msg.  r (wsg_reply_messages): the plan
// with the reply frames' geometry scanned behind it, then the same gather, its
// destination the reply wire.
int messages(wsg_ctx* c, const wsg::Batch& b, wsg_stream_state* d_state, uint8_t* d_msg, uint64_t msg_cap,
             const wsg::ReplyOut* r, const wsg::MsgOut& o, void* stream)
{
    if (!c || wsg::args_messages(b, d_state, d_msg, msg_cap, r, o, nullptr, nullptr, nullptr, nullptr, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    wsg::MsgScratch x;
    bool ordered = false;
    if (int rc = msg_scratch(c, s, b.n, b.wire_len, &x, &ordered))
        return rc;
    WSG_HIP(r ? wsg::launch_reply_plan(s, b, d_state, *r, o, x)
              : wsg::launch_msg_plan(s, b, d_state, d_state, msg_cap, o, x));
    if (b.n)
        if (int rc = r ? gather_launch(c, s, b.wire, x.plans.ref.rtot, x, r->reply, r->reply_cap)
                       : gather_launch(c, s, b.wire, x.plans.ref.tot, x, d_msg, msg_cap))
            return rc;
    return scratch_leave(c->msg_order, s, ordered);
}

} // namespace

int wsg_decode_messages(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start,
                        uint32_t n, const uint32_t* d_stream_first, uint32_t n_streams, wsg_stream_state* d_state,
                        uint8_t* d_msg, uint64_t msg_cap, wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                        void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    return messages(c, b, d_state, d_msg, msg_cap, nullptr, wsg::MsgOut{d_msgs, d_count, d_info}, stream);
}

// UTF-8 over the messages of a decode: one lane per record before and behind
// the payload kernel, which reads every byte of d_msg below the bound once.
int wsg_check_utf8(wsg_ctx* c, const uint8_t* d_msg, uint64_t msg_cap, const wsg_msg* d_msgs, const uint64_t* d_count,
                   uint32_t msg_room, uint32_t which, uint64_t* d_valid, uint64_t* d_result, void* stream)
{
    if (!c || wsg::args_check_utf8(d_msg, msg_cap, d_msgs, d_count, msg_room, d_valid, d_result, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    const int rec_grid = grid_for(c, ceil_div(msg_room, wsg::BLOCK));   // (at least one block: it seeds d_result)
    WSG_HIP(wsg::launch_utf8_init(s, rec_grid, d_msgs, d_count, msg_room, d_valid, d_result));
    if (msg_room == 0)
        return WSG_OK;
    if (which && msg_cap) {
        const int t = timing_begin(c, s);
        WSG_HIP(wsg::launch_utf8_scan(s, grid_for(c, ceil_div(msg_cap, uint64_t(wsg::BLOCK) * wsg::CHUNK), c->utf8_blocks_per_cu),
                                      d_msg, msg_cap, d_msgs, d_count, msg_room, which, d_valid));
        timing_end(c, s, t);
    }
    WSG_HIP(wsg::launch_utf8_count(s, rec_grid, d_msgs, d_count, msg_room, msg_cap, which, d_valid, d_result));
    return WSG_OK;
}

// wsg_check_utf8 with the message plan in front of it and the wire in the
// place of d_msg: the plan up to the piece records (d_state only read), the
// per-record kernels around the payload kernel, which reads every delivered
// payload byte once where it lies.
int wsg_check_utf8_wire(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start,
                        uint32_t n, const uint32_t* d_stream_first, uint32_t n_streams,
                        const wsg_stream_state* d_state, uint32_t which, wsg_msg* d_msgs, uint64_t* d_count,
                        wsg_recv_info* d_info, uint64_t* d_valid, uint64_t* d_result, void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    const wsg::MsgOut o{d_msgs, d_count, d_info};
    const wsg::Utf8Inside u{which, d_valid, d_result, /*also*/ nullptr, /*grids*/ 1, 1};
    if (!c || wsg::args_messages(b, d_state, nullptr, 0, nullptr, o, nullptr, &u, nullptr, nullptr, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    wsg::MsgScratch x;
    bool ordered = false;
    if (int rc = msg_scratch(c, s, n, wire_len, &x, &ordered))
        return rc;
    WSG_HIP(wsg::launch_msg_plan(s, b, nullptr, d_state, UINT64_MAX, o, x));
    const int rec_grid = grid_for(c, ceil_div(n, wsg::BLOCK));   // (at least one block: it seeds d_result)
    WSG_HIP(wsg::launch_utf8_init(s, rec_grid, d_msgs, d_count, n, d_valid, d_result));
    if (n && which) {
        const int t = timing_begin(c, s);
        WSG_HIP(wsg::launch_utf8_wire(s, piece_grid(c, x.pieces_cap, c->utf8_wire_blocks_per_cu), b, o, x, which,
                                      d_valid));
        timing_end(c, s, t);
    }
    WSG_HIP(wsg::launch_utf8_count(s, rec_grid, d_msgs, d_count, n, UINT64_MAX, which, d_valid, d_result));
    return scratch_leave(c->msg_order, s, ordered);
}

// The frame-sequence rules over a decoded batch: a scan of the frames' steps
// on their stream's state, the judging kernel (one lane per frame), one lane
// per stream behind it.
int wsg_check_protocol(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const wsg_recv_info* d_info, uint32_t n,
                       const uint32_t* d_stream_first, uint32_t n_streams, const wsg_stream_state* d_state,
                       wsg_proto_state* d_proto, uint32_t role, uint64_t max_message, wsg_proto_verdict* d_verdict,
                       uint64_t* d_result, void* stream)
{
    const wsg::Batch b{d_wire, wire_len, /*fs*/ nullptr, n, d_stream_first, n_streams};
    const wsg::ProtoOps p{d_proto, role, max_message, /*also*/ nullptr, d_verdict, d_result};
    if (!c || wsg::args_check_protocol(b, d_info, d_state, p, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    wsg::ProtoPlan plan;
    bool ordered = false;
    if (int rc = proto_scratch(c, s, n, n_streams, &plan, &ordered))
        return rc;
    WSG_HIP(wsg::launch_proto_scan(s, b, d_info, p, plan));
    if (n && n_streams) {
        const int t = timing_begin(c, s);
        WSG_HIP(wsg::launch_proto_judge(s, b, d_info, d_state, p, plan));
        timing_end(c, s, t);
    }
    WSG_HIP(wsg::launch_proto_finish(s, grid_for(c, ceil_div(n_streams, wsg::BLOCK)), b, d_state, p, plan));
    return scratch_leave(c->proto_order, s, ordered);
}

// The device framer: two walks over every stream (one wave each) with a scan
// of the per-stream frame counts between them.
int wsg_frame_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                      uint32_t n_streams, uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                      uint64_t* d_count, void* stream)
{
    if (!c || wsg::args_frame_streams(d_wire, wire_len, d_span, n_streams, d_frame_start, frame_cap, d_stream_first,
                                      d_count, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    if (int rc = ensure_array(c->d_frame_plan, c->frame_plan_cap, wsg::frame_plan_layout(nullptr, n_streams, nullptr)))
        return rc;
    wsg::FramePlan plan;
    wsg::frame_plan_layout(c->d_frame_plan, n_streams, &plan);
    // the counts and partials are the context's: behind the previous call's
    // kernels, whatever stream they ran on
    bool ordered = false;
    if (int rc = scratch_enter(c->frame_order, s, &ordered))
        return rc;
    const int t = n_streams ? timing_begin(c, s) : -1;
    WSG_HIP(wsg::launch_frame_streams(s, grid_for(c, ceil_div(n_streams, wsg::BLOCK / 64), c->dec_blocks_per_cu), d_wire,
                                      wire_len, d_span, n_streams, d_frame_start, frame_cap, d_stream_first, d_count,
                                      plan, c->d_err));
    timing_end(c, s, t);
    return scratch_leave(c->frame_order, s, ordered);
}

// The upgrade handshake: one wave per stream judges the request, a scan of the
// response sizes, the accept values, the responses.  The framer's scratch and
// its order: a connection is in front of one call or the other.
int wsg_upgrade_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                        uint32_t n_streams, uint64_t max_request, wsg_upgrade* d_up, uint8_t* d_resp,
                        uint64_t resp_cap, uint64_t* d_resp_off, uint64_t* d_count, void* stream)
{
    if (!c || wsg::args_upgrade_streams(d_wire, wire_len, d_span, n_streams, d_up, d_resp, resp_cap, d_resp_off,
                                        d_count, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    if (int rc = ensure_array(c->d_frame_plan, c->frame_plan_cap, wsg::upgrade_plan_layout(nullptr, n_streams, nullptr)))
        return rc;
    wsg::UpgradePlan plan;
    wsg::upgrade_plan_layout(c->d_frame_plan, n_streams, &plan);
    bool ordered = false;
    if (int rc = scratch_enter(c->frame_order, s, &ordered))
        return rc;
    const int t = n_streams ? timing_begin(c, s) : -1;
    WSG_HIP(wsg::launch_upgrade_streams(s, grid_for(c, ceil_div(n_streams, wsg::BLOCK / 64), c->dec_blocks_per_cu),
                                        d_wire, wire_len, d_span, n_streams, max_request, d_up, d_resp, resp_cap,
                                        d_resp_off, d_count, plan, c->d_err));
    timing_end(c, s, t);
    return scratch_leave(c->frame_order, s, ordered);
}

// The client's half of the handshake: the streams' expected digests, one wave
// per stream judges the response, the counts.  The framer's scratch and its
// order, as wsg_upgrade_streams.
int wsg_upgrade_client_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                               uint32_t n_streams, const uint8_t* d_nonce, uint64_t max_response,
                               wsg_upgrade_reply* d_up, uint64_t* d_count, void* stream)
{
    if (!c || wsg::args_upgrade_client(d_wire, wire_len, d_span, n_streams, d_nonce, d_up, d_count, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    if (int rc = ensure_array(c->d_frame_plan, c->frame_plan_cap, wsg::upclient_plan_layout(nullptr, n_streams, nullptr)))
        return rc;
    wsg::UpClientPlan plan;
    wsg::upclient_plan_layout(c->d_frame_plan, n_streams, &plan);
    bool ordered = false;
    if (int rc = scratch_enter(c->frame_order, s, &ordered))
        return rc;
    const int t = n_streams ? timing_begin(c, s) : -1;
    WSG_HIP(wsg::launch_upgrade_client_streams(s, grid_for(c, ceil_div(n_streams, wsg::BLOCK / 64), c->dec_blocks_per_cu),
                                               d_wire, wire_len, d_span, n_streams, d_nonce, max_response, d_up,
                                               d_count, plan, c->d_err));
    timing_end(c, s, t);
    return scratch_leave(c->frame_order, s, ordered);
}

// The requests of those nonces: one kernel, a 16-byte block of d_req per lane.
// Twice through the arguments, as the fan-out: the capacity has its turn
// before the allocations are looked up.
int wsg_upgrade_requests(wsg_ctx* c, const uint8_t* d_tpl, uint32_t tpl_len, uint32_t key_at, const uint8_t* d_nonce,
                         uint32_t n, uint8_t* d_req, uint64_t req_cap, void* stream)
{
    const uint64_t total = uint64_t(n) * tpl_len;
    if (!c || wsg::args_upgrade_requests(d_tpl, tpl_len, key_at, d_nonce, n, d_req, total, false))
        return WSG_EINVAL;
    if (total > req_cap)
        return WSG_ENOMEM;
    if (wsg::args_upgrade_requests(d_tpl, tpl_len, key_at, d_nonce, n, d_req, total, c->check))
        return WSG_EINVAL;
    if (n == 0)
        return WSG_OK;
    hipStream_t s = as_stream(stream);
    const int t = timing_begin(c, s);
    WSG_HIP(wsg::launch_upgrade_requests(s, grid_for(c, ceil_div(ceil_div(total, uint64_t(wsg::CHUNK)), wsg::BLOCK)),
                                         d_tpl, tpl_len, key_at, d_nonce, d_req, total));
    timing_end(c, s, t);
    return WSG_OK;
}

// The carry: per-stream sizes and a scan (one lane per stream), then the copy,
// which writes every 16-byte chunk of the next wire once.  The framer's
// scratch and its order: a round is one call or the other at a time.
int wsg_carry_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const wsg_stream_span* d_span,
                      uint32_t n_streams, const uint64_t* d_close_off, const uint8_t* d_new, uint64_t new_len,
                      const wsg_stream_read* d_read, uint8_t* d_next, uint64_t next_cap, wsg_stream_span* d_next_span,
                      uint64_t* d_count, void* stream)
{
    if (!c || wsg::args_carry_streams(d_wire, wire_len, d_span, n_streams, d_close_off, d_new, new_len, d_read, d_next,
                                      next_cap, d_next_span, d_count, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    if (int rc = ensure_array(c->d_frame_plan, c->frame_plan_cap, wsg::carry_plan_layout(nullptr, n_streams, nullptr)))
        return rc;
    wsg::CarryPlan plan;
    wsg::carry_plan_layout(c->d_frame_plan, n_streams, &plan);
    bool ordered = false;
    if (int rc = scratch_enter(c->frame_order, s, &ordered))
        return rc;
    WSG_HIP(wsg::launch_carry_plan(s, wire_len, d_span, n_streams, d_close_off, new_len, d_read, next_cap, d_next_span,
                                   d_count, plan, c->d_err));
    // the pieces the copy can have: a stream adds less than a chunk of padding
    // to its bytes, and a total above next_cap writes nothing
    const uint64_t most = std::min(next_cap, wire_len + new_len + uint64_t(n_streams) * wsg::CHUNK);
    if (n_streams && most) {
        const int t = timing_begin(c, s);
        WSG_HIP(wsg::launch_carry_copy(s, piece_grid(c, ceil_div(most, wsg::PIECE), c->dec_blocks_per_cu), d_wire,
                                       d_new, n_streams, plan, d_next, next_cap));
        timing_end(c, s, t);
    }
    return scratch_leave(c->frame_order, s, ordered);
}

namespace {

// The _streams forms: the framer, one synchronisation to read the frame
// count, `messages(the batch of the frames it found)`, the spans' consumed
// lowered to the first tail frame.  b: the batch at n = f.frame_cap, which the
// caller has checked.
template <class Messages>
int streams_then(wsg_ctx* c, const wsg::Batch& b, const wsg::Framed& f, wsg_stream_state* d_state, uint64_t* d_count,
                 void* stream, Messages messages)
{
    hipStream_t s = as_stream(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    WSG_HIP(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return WSG_EINVAL;   // the frame count is read on the host in the middle
    *f.n_frames_out = 0;
    if (int rc = wsg_frame_streams(c, b.wire, b.wire_len, f.span, b.n_streams, f.frame_start, f.frame_cap,
                                   f.stream_first, d_count, stream))
        return rc;
    uint64_t found = 0;
    WSG_HIP(hipMemcpyAsync(&found, d_count, sizeof(found), hipMemcpyDeviceToHost, s));
    WSG_HIP(hipStreamSynchronize(s));
    if (found > uint64_t(UINT32_MAX) - 1)
        return WSG_EINVAL;
    if (found > f.frame_cap)
        return WSG_ENOMEM;
    wsg::Batch frames = b;
    frames.n = uint32_t(found);
    *f.n_frames_out = frames.n;
    if (int rc = messages(frames))
        return rc;
    WSG_HIP(wsg::launch_frame_tail(s, f.span, b.n_streams, f.frame_start, f.stream_first, d_state, frames.n));
    return WSG_OK;
}

} // namespace

int wsg_decode_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                       uint32_t n_streams, wsg_stream_state* d_state, uint64_t* d_frame_start, uint32_t frame_cap,
                       uint32_t* d_stream_first, uint8_t* d_msg, uint64_t msg_cap, wsg_msg* d_msgs, uint64_t* d_count,
                       wsg_recv_info* d_info, uint32_t* n_frames_out, void* stream)
{
    const wsg::Framed f{d_span, d_frame_start, frame_cap, d_stream_first, n_frames_out};
    // (every frame the framer has room for)
    const wsg::Batch b{d_wire, wire_len, f.frame_start, f.frame_cap, f.stream_first, n_streams};
    const wsg::MsgOut o{d_msgs, d_count, d_info};
    if (!c || wsg::args_messages(b, d_state, d_msg, msg_cap, nullptr, o, nullptr, nullptr, nullptr, &f, c->check))
        return WSG_EINVAL;
    return streams_then(c, b, f, d_state, d_count, stream, [&](const wsg::Batch& frames) {
        return messages(c, frames, d_state, d_msg, msg_cap, nullptr, o, stream);
    });
}

namespace {

// wsg_reply_messages with wsg_check_protocol inside it: the protocol kernels
// run on the d_info the plan's header pass has just written, and the reply
// kernels stop every stream at its terminal frame and close it there.
// utf8 (wsg_reply_validated): the UTF-8 check from the wire inside the plan,
// d_valid and d_utf8_result written, its verdicts merged with p.also.
// relay (wsg_relay_validated): the relay's plan and gather behind the reply side.
int reply_checked(wsg_ctx* c, const wsg::Batch& b, wsg_stream_state* d_state, const wsg::ProtoOps& p,
                  const wsg::ReplyOut& r, const wsg::MsgOut& o, const wsg::Utf8Inside* utf8,
                  const wsg::RelayArgs* relay, void* stream)
{
    if (!c || wsg::args_messages(b, d_state, nullptr, 0, &r, o, &p, utf8, relay, nullptr, c->check))
        return WSG_EINVAL;
    bool relays = false;   // a kind is relayed: the relay's gather has something to move
    for (int k = 1; relay && k < 5; ++k)
        relays = relays || relay->relay_op[k];
    hipStream_t s = as_stream(stream);
    // both scratches are the context's: behind the last user of either,
    // whatever stream it ran on
    wsg::ProtoPlan pplan;
    wsg::MsgScratch x;
    bool ordered = false, pordered = false;
    wsg::Utf8Inside u = utf8 ? *utf8 : wsg::Utf8Inside{};
    if (int rc = proto_scratch(c, s, b.n, b.n_streams, &pplan, &pordered, utf8 ? &u.also : nullptr))
        return rc;
    if (int rc = msg_scratch(c, s, b.n, b.wire_len, &x, &ordered))
        return rc;
    wsg::RelayPlan rplan;
    if (relay)
        if (int rc = relay_scratch(c, b.n, b.n_streams, x.pieces_cap, &rplan))
            return rc;
    u.rec_grid = grid_for(c, ceil_div(b.n, wsg::BLOCK));
    u.wire_grid = piece_grid(c, x.pieces_cap, c->utf8_wire_blocks_per_cu);
    WSG_HIP(wsg::launch_reply_checked_plan(s, grid_for(c, ceil_div(b.n_streams, wsg::BLOCK)), b, d_state, p, pplan, r,
                                           o, x, utf8 ? &u : nullptr));
    if (b.n)
        if (int rc = gather_launch(c, s, b.wire, x.plans.ref.rtot, x, r.reply, r.reply_cap))
            return rc;
    if (relay) {
        // behind the whole reply side, which it reads (d_info, d_msgs, d_verdict) and leaves as it is
        wsg::MsgScratch rx = x;
        rx.pieces = c->d_relay_pieces;
        WSG_HIP(wsg::launch_relay_plan(s, b, o, p.verdict, *relay, rplan, rx));
        if (b.n && relays)
            if (int rc = gather_launch(c, s, b.wire, rplan.gtot, rx, relay->relay, relay->relay_cap))
                return rc;
    }
    if (int rc = scratch_leave(c->proto_order, s, pordered))
        return rc;
    return scratch_leave(c->msg_order, s, ordered);
}

// The _streams form of the replies: of messages() (p null) and of reply_checked.
int reply_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, uint32_t n_streams, const wsg::Framed& f,
                  wsg_stream_state* d_state, const wsg::ProtoOps* p, const wsg::ReplyOut& r, const wsg::MsgOut& o,
                  const wsg::Utf8Inside* utf8, const wsg::RelayArgs* relay, void* stream)
{
    // (every frame the framer has room for)
    const wsg::Batch b{d_wire, wire_len, f.frame_start, f.frame_cap, f.stream_first, n_streams};
    if (!c || wsg::args_messages(b, d_state, nullptr, 0, &r, o, p, utf8, relay, &f, c->check))
        return WSG_EINVAL;
    return streams_then(c, b, f, d_state, o.count, stream, [&](const wsg::Batch& frames) {
        return p ? reply_checked(c, frames, d_state, *p, r, o, utf8, relay, stream)
                 : messages(c, frames, d_state, nullptr, 0, &r, o, stream);
    });
}

} // namespace

int wsg_reply_messages(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start, uint32_t n,
                       const uint32_t* d_stream_first, uint32_t n_streams, wsg_stream_state* d_state,
                       const uint8_t reply_op[5], int mask, const uint32_t* d_send_key, uint8_t* d_reply,
                       uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply, wsg_msg* d_msgs,
                       uint64_t* d_count, wsg_recv_info* d_info, void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply,
                          /*close_off*/ nullptr};
    return messages(c, b, d_state, nullptr, 0, &r, wsg::MsgOut{d_msgs, d_count, d_info}, stream);
}

int wsg_reply_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                      uint32_t n_streams, wsg_stream_state* d_state, uint64_t* d_frame_start, uint32_t frame_cap,
                      uint32_t* d_stream_first, const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                      uint8_t* d_reply, uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply,
                      wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info, uint32_t* n_frames_out, void* stream)
{
    const wsg::Framed f{d_span, d_frame_start, frame_cap, d_stream_first, n_frames_out};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply,
                          /*close_off*/ nullptr};
    return reply_streams(c, d_wire, wire_len, n_streams, f, d_state, nullptr, r, wsg::MsgOut{d_msgs, d_count, d_info},
                         nullptr, nullptr, stream);
}

int wsg_reply_checked(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start, uint32_t n,
                      const uint32_t* d_stream_first, uint32_t n_streams, wsg_stream_state* d_state,
                      wsg_proto_state* d_proto, uint32_t role, uint64_t max_message, const wsg_proto_verdict* d_also,
                      const uint8_t reply_op[5], int mask, const uint32_t* d_send_key, uint8_t* d_reply,
                      uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                      wsg_proto_verdict* d_verdict, uint64_t* d_result, wsg_msg* d_msgs, uint64_t* d_count,
                      wsg_recv_info* d_info, void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    const wsg::ProtoOps p{d_proto, role, max_message, d_also, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    return reply_checked(c, b, d_state, p, r, wsg::MsgOut{d_msgs, d_count, d_info}, nullptr, nullptr, stream);
}

// wsg_reply_checked with wsg_check_utf8_wire and wsg_utf8_verdicts inside its
// plan: one plan pass, the payload read once for the check and once for the
// reply, written once.
int wsg_reply_validated(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start,
                        uint32_t n, const uint32_t* d_stream_first, uint32_t n_streams, wsg_stream_state* d_state,
                        wsg_proto_state* d_proto, uint32_t role, uint64_t max_message, const wsg_proto_verdict* d_also,
                        uint32_t which, const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                        uint8_t* d_reply, uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply,
                        uint64_t* d_close_off, wsg_proto_verdict* d_verdict, uint64_t* d_result, uint64_t* d_valid,
                        uint64_t* d_utf8_result, wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                        void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    const wsg::ProtoOps p{d_proto, role, max_message, d_also, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    const wsg::Utf8Inside u{which, d_valid, d_utf8_result, /*also*/ nullptr, /*grids*/ 1, 1};
    return reply_checked(c, b, d_state, p, r, wsg::MsgOut{d_msgs, d_count, d_info}, &u, nullptr, stream);
}

int wsg_reply_checked_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                              uint32_t n_streams, wsg_stream_state* d_state, uint64_t* d_frame_start,
                              uint32_t frame_cap, uint32_t* d_stream_first, wsg_proto_state* d_proto, uint32_t role,
                              uint64_t max_message, const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                              uint8_t* d_reply, uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply,
                              uint64_t* d_close_off, wsg_proto_verdict* d_verdict, uint64_t* d_result, wsg_msg* d_msgs,
                              uint64_t* d_count, wsg_recv_info* d_info, uint32_t* n_frames_out, void* stream)
{
    const wsg::Framed f{d_span, d_frame_start, frame_cap, d_stream_first, n_frames_out};
    const wsg::ProtoOps p{d_proto, role, max_message, /*also*/ nullptr, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    return reply_streams(c, d_wire, wire_len, n_streams, f, d_state, &p, r, wsg::MsgOut{d_msgs, d_count, d_info},
                         nullptr, nullptr, stream);
}

int wsg_reply_validated_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                                uint32_t n_streams, wsg_stream_state* d_state, uint64_t* d_frame_start,
                                uint32_t frame_cap, uint32_t* d_stream_first, wsg_proto_state* d_proto, uint32_t role,
                                uint64_t max_message, uint32_t which, const uint8_t reply_op[5], int mask,
                                const uint32_t* d_send_key, uint8_t* d_reply, uint64_t reply_cap,
                                uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                                wsg_proto_verdict* d_verdict, uint64_t* d_result, uint64_t* d_valid,
                                uint64_t* d_utf8_result, wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                                uint32_t* n_frames_out, void* stream)
{
    const wsg::Framed f{d_span, d_frame_start, frame_cap, d_stream_first, n_frames_out};
    const wsg::ProtoOps p{d_proto, role, max_message, /*also*/ nullptr, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    const wsg::Utf8Inside u{which, d_valid, d_utf8_result, /*also*/ nullptr, /*grids*/ 1, 1};
    return reply_streams(c, d_wire, wire_len, n_streams, f, d_state, &p, r, wsg::MsgOut{d_msgs, d_count, d_info}, &u,
                         nullptr, stream);
}

// wsg_reply_validated with the relay's plan and gather behind it: the reply
// side runs as it does there, then every relayed message is sized, placed by
// room and moved once into d_relay.
int wsg_relay_validated(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start,
                        uint32_t n, const uint32_t* d_stream_first, uint32_t n_streams, wsg_stream_state* d_state,
                        wsg_proto_state* d_proto, uint32_t role, uint64_t max_message, const wsg_proto_verdict* d_also,
                        uint32_t which, const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                        const uint8_t relay_op[5], const uint32_t* d_order, const uint32_t* d_group_first,
                        uint32_t n_groups, uint8_t* d_reply, uint64_t reply_cap, uint64_t* d_reply_off,
                        uint64_t* d_stream_reply, uint64_t* d_close_off, uint8_t* d_relay, uint64_t relay_cap,
                        uint64_t* d_relay_off, uint64_t* d_group_relay, wsg_proto_verdict* d_verdict,
                        uint64_t* d_result, uint64_t* d_valid, uint64_t* d_utf8_result, wsg_msg* d_msgs,
                        uint64_t* d_count, wsg_recv_info* d_info, void* stream)
{
    const wsg::Batch b{d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams};
    const wsg::ProtoOps p{d_proto, role, max_message, d_also, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    const wsg::Utf8Inside u{which, d_valid, d_utf8_result, /*also*/ nullptr, /*grids*/ 1, 1};
    const wsg::RelayArgs relay{relay_op, d_order, d_group_first, n_groups, d_relay, relay_cap, d_relay_off, d_group_relay};
    return reply_checked(c, b, d_state, p, r, wsg::MsgOut{d_msgs, d_count, d_info}, &u, &relay, stream);
}

int wsg_relay_validated_streams(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, wsg_stream_span* d_span,
                                uint32_t n_streams, wsg_stream_state* d_state, uint64_t* d_frame_start,
                                uint32_t frame_cap, uint32_t* d_stream_first, wsg_proto_state* d_proto, uint32_t role,
                                uint64_t max_message, uint32_t which, const uint8_t reply_op[5], int mask,
                                const uint32_t* d_send_key, const uint8_t relay_op[5], const uint32_t* d_order,
                                const uint32_t* d_group_first, uint32_t n_groups, uint8_t* d_reply,
                                uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply,
                                uint64_t* d_close_off, uint8_t* d_relay, uint64_t relay_cap, uint64_t* d_relay_off,
                                uint64_t* d_group_relay, wsg_proto_verdict* d_verdict, uint64_t* d_result,
                                uint64_t* d_valid, uint64_t* d_utf8_result, wsg_msg* d_msgs, uint64_t* d_count,
                                wsg_recv_info* d_info, uint32_t* n_frames_out, void* stream)
{
    const wsg::Framed f{d_span, d_frame_start, frame_cap, d_stream_first, n_frames_out};
    const wsg::ProtoOps p{d_proto, role, max_message, /*also*/ nullptr, d_verdict, d_result};
    const wsg::ReplyOut r{reply_op, mask, d_send_key, d_reply, reply_cap, d_reply_off, d_stream_reply, d_close_off};
    const wsg::Utf8Inside u{which, d_valid, d_utf8_result, /*also*/ nullptr, /*grids*/ 1, 1};
    const wsg::RelayArgs relay{relay_op, d_order, d_group_first, n_groups, d_relay, relay_cap, d_relay_off, d_group_relay};
    return reply_streams(c, d_wire, wire_len, n_streams, f, d_state, &p, r, wsg::MsgOut{d_msgs, d_count, d_info}, &u,
                         &relay, stream);
}

// wsg_check_utf8's d_valid as the d_also of wsg_reply_checked: a seed per
// stream, then one lane per record.
int wsg_utf8_verdicts(wsg_ctx* c, const wsg_msg* d_msgs, const uint64_t* d_count, uint32_t msg_room, uint32_t which,
                      const uint64_t* d_valid, uint32_t n_streams, wsg_proto_verdict* d_also, void* stream)
{
    if (!c || wsg::args_utf8_verdicts(d_msgs, d_count, msg_room, d_valid, n_streams, d_also, c->check))
        return WSG_EINVAL;
    if (n_streams == 0)
        return WSG_OK;
    WSG_HIP(wsg::launch_utf8_verdicts(as_stream(stream), grid_for(c, ceil_div(msg_room, wsg::BLOCK)),
                                      grid_for(c, ceil_div(n_streams, wsg::BLOCK)), d_msgs, d_count, msg_room, which,
                                      d_valid, n_streams, d_also));
    return WSG_OK;
}

namespace {

// Small-frame batches (average frame <= small_avg) take k_encode_small,
// the rest the piece kernel.
bool small_path(const wsg_ctx* c, uint32_t n, uint64_t wire_cap) { return wire_cap <= uint64_t(n) * c->small_avg; }

} // namespace

int ensure_enc(const wsg_ctx* c, wsg_enc_scratch& e, uint32_t n, uint64_t wire_cap)
{
    if (int rc = ensure_array(e.d_scan, e.scan_cap, 4 * ceil_div(n, wsg::SCAN_ITEMS)))
        return rc;
    if (int rc = ensure_array(e.d_piece_start, e.piece_start_cap, uint64_t(n) + 1))
        return rc;
    if (c && small_path(c, n, wire_cap))
        return WSG_OK;
    // pieces are indexed by u32 in the launch (q_begin / q_end): a bound past
    // that (a wire_cap of terabytes, far past any HBM) is refused, not wrapped
    if (pieces_bound(n, wire_cap) > UINT32_MAX)
        return WSG_EINVAL;
    return ensure_array(e.d_piece_frame, e.piece_frame_cap, pieces_bound(n, wire_cap));
}

int encode_launch(wsg_ctx* c, hipStream_t s, const uint8_t* d_payload, const wsg_send_desc* d_desc, uint32_t n,
                  uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off, wsg_enc_scratch& e,
                  unsigned long long* err)
{
    if (small_path(c, n, wire_cap)) {   // sizes scan, then one block per group of frames
        WSG_HIP(wsg::launch_encode_scan_small(s, d_desc, n, d_wire_off, e.d_scan));
        const int t = timing_begin(c, s);
        WSG_HIP(wsg::launch_encode_small(s, d_payload, d_desc, n, d_wire_off, e.d_scan, d_wire, wire_cap, err));
        timing_end(c, s, t);
        return WSG_OK;
    }
    const uint64_t pieces_cap = pieces_bound(n, wire_cap);
    if (pieces_cap > UINT32_MAX)   // as ensure_enc: u32 piece indices below
        return WSG_EINVAL;
    WSG_HIP(wsg::launch_encode_scan(s, d_desc, n, d_wire_off, e.d_piece_start, e.d_scan, e.d_piece_frame, pieces_cap,
                                    wire_cap, err));
    // one launch per run of at most enc_launch_pieces pieces (0: one launch)
    const uint64_t per = c->enc_launch_pieces ? c->enc_launch_pieces : pieces_cap;
    const int t = timing_begin(c, s);
    for (uint64_t q0 = 0; q0 < pieces_cap; q0 += per) {
        const uint64_t q1 = std::min<uint64_t>(pieces_cap, q0 + per);
        WSG_HIP(wsg::launch_encode_mask(s, piece_grid(c, q1 - q0, c->enc_blocks_per_cu),
                                        d_payload, d_desc, n, d_wire_off, e.d_piece_start, e.d_piece_frame, d_wire,
                                        wire_cap, uint32_t(q0), uint32_t(q1)));
    }
    timing_end(c, s, t);
    return WSG_OK;
}

int wsg_encode_batch(wsg_ctx* c, const uint8_t* d_payload, const wsg_send_desc* d_desc, uint32_t n, uint8_t* d_wire,
                     uint64_t wire_cap, uint64_t* d_wire_off, void* stream)
{
    if (!c || wsg::args_encode_batch(d_desc, n, d_wire, wire_cap, d_wire_off, c->check))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    if (n == 0) {
        WSG_HIP(hipMemsetAsync(d_wire_off, 0, sizeof(uint64_t), s));
        return WSG_OK;
    }
    if (c->check) {   // the descriptors come to the host: every payload range
        std::vector<wsg_send_desc> h;
        try {
            h.resize(n);
        } catch (...) {
            return WSG_ENOMEM;
        }
        WSG_HIP(hipMemcpyAsync(h.data(), d_desc, uint64_t(n) * sizeof(wsg_send_desc), hipMemcpyDeviceToHost, s));
        WSG_HIP(hipStreamSynchronize(s));
        for (const wsg_send_desc& d : h)
            if (d.len && (!d_payload || !in_alloc(d_payload + d.src_off, d.len)))
                return WSG_EINVAL;
    }
    if (int rc = ensure_enc(c, c->enc, n, wire_cap))
        return rc;
    // c->enc is the context's: behind the previous call's kernels, whatever
    // stream they ran on
    bool ordered = false;
    if (int rc = scratch_enter(c->enc_order, s, &ordered))
        return rc;
    if (int rc = encode_launch(c, s, d_payload, d_desc, n, d_wire, wire_cap, d_wire_off, c->enc, c->d_err))
        return rc;
    return scratch_leave(c->enc_order, s, ordered);
}

namespace {

// One fan-out message's k frames on the flat / piece kernels (frame sizes the
// period path does not take).
int fanout_one_flat(wsg_ctx* c, hipStream_t s, const uint8_t* d_payload, uint64_t len, const uint32_t* d_keys,
                    uint32_t k, uint8_t opcode, int mask, uint8_t* d_wire)
{
    const uint64_t fsize = wsg_frame_size(opcode, mask, len, 0);
    const uint64_t total = fsize * k;
    const uint64_t blocks = ceil_div(ceil_div(total, wsg::CHUNK), wsg::BLOCK * wsg::FAN_UNITS);
    WSG_HIP(wsg::launch_fanout(s, grid_for(c, blocks), d_payload, len, d_keys, k, opcode, mask ? 1u : 0u, fsize,
                               d_wire));
    return WSG_OK;
}

// m messages x k keys.  Messages of one geometry (length, opcode) whose frame
// size suits the period kernel go FAN_MSGS at a time into one launch
// (blockIdx.y = message); the others take one flat launch each.
int fanout_many(wsg_ctx* c, hipStream_t s, const uint8_t* d_payload, const uint64_t* src_off, const uint64_t* len,
                const uint8_t* opcode, uint32_t m, const uint32_t* d_keys, uint32_t k, int mask, uint8_t* d_wire,
                const uint64_t* wire_off)
{
    std::vector<char> done(m, 0);
    for (uint32_t i = 0; i < m; ++i) {
        if (done[i])
            continue;
        const uint64_t fsize = wsg_frame_size(opcode[i], mask, len[i], 0);
        wsg::FanMsgs g{};
        uint32_t cnt = 0;
        std::vector<uint32_t> members;
        for (uint32_t q = i; q < m; ++q) {
            if (done[q] || len[q] != len[i] || opcode[q] != opcode[i])
                continue;
            members.push_back(q);
        }
        for (size_t at = 0; at < members.size(); at += wsg::FAN_MSGS) {
            cnt = uint32_t(std::min<size_t>(wsg::FAN_MSGS, members.size() - at));
            for (uint32_t q = 0; q < cnt; ++q) {
                g.src[q] = src_off[members[at + q]];
                g.dst[q] = wire_off[members[at + q]];
            }
            hipError_t perr = hipSuccess;
            if (wsg::launch_fanout_period(s, c->num_cus, c->fan_waves_per_cu, c->fan_wpb, d_payload, len[i], d_keys, k, opcode[i],
                                          mask ? 1u : 0u, fsize, d_wire, g, cnt, &perr)) {
                WSG_HIP(perr);
            } else {
                for (uint32_t q = 0; q < cnt; ++q)
                    if (int rc = fanout_one_flat(c, s, d_payload + g.src[q], len[i], d_keys, k, opcode[i], mask,
                                                 d_wire + g.dst[q]))
                        return rc;
            }
        }
        for (uint32_t q : members)
            done[q] = 1;
    }
    return WSG_OK;
}

} // namespace

int wsg_fanout_encode(wsg_ctx* c, const uint8_t* d_payload, uint64_t len, const uint32_t* d_keys, uint32_t k,
                      uint8_t opcode, int mask, uint8_t* d_wire, uint64_t wire_cap, void* stream)
{
    const uint64_t total = wsg_frame_size(opcode, mask, len, 0) * k;
    if (!c || wsg::args_fanout_encode(d_payload, len, d_keys, k, d_wire, total, false))
        return WSG_EINVAL;
    if (k == 0)
        return WSG_OK;
    if (total > wire_cap)
        return WSG_ENOMEM;
    if (c->check && wsg::args_fanout_encode(d_payload, len, d_keys, k, d_wire, total, true))
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    const uint64_t src = 0, off[2] = {0, total};
    const int t = timing_begin(c, s);
    if (int rc = fanout_many(c, s, d_payload, &src, &len, &opcode, 1, d_keys, k, mask, d_wire, off))
        return rc;
    timing_end(c, s, t);
    return WSG_OK;
}

int wsg_fanout_encode_many(wsg_ctx* c, const uint8_t* d_payload, const uint64_t* src_off, const uint64_t* len,
                           const uint8_t* opcode, uint32_t m, const uint32_t* d_keys, uint32_t k, int mask,
                           uint8_t* d_wire, uint64_t wire_cap, uint64_t* wire_off, void* stream)
{
    try {   // no C++ exception leaves the ABI (host vectors: WSG_ENOMEM)
        if (!c || wsg::args_fanout_encode_many(src_off, len, opcode, m, d_keys, k, d_wire, 0, wire_off, false))
            return WSG_EINVAL;
        // message i's frames from wire_off[i], line-aligned (whole-line store rows)
        uint64_t at = 0;
        bool any_payload = false;
        for (uint32_t i = 0; i < m; ++i) {
            at = (at + wsg::PIECE_ALIGN - 1) & ~(wsg::PIECE_ALIGN - 1);
            wire_off[i] = at;
            at += wsg_frame_size(opcode[i], mask, len[i], 0) * k;
            any_payload = any_payload || len[i] != 0;
        }
        wire_off[m] = at;
        if (at > wire_cap)
            return WSG_ENOMEM;
        if (m == 0 || k == 0)
            return WSG_OK;
        if (any_payload && !d_payload)
            return WSG_EINVAL;
        if (c->check) {
            if (wsg::args_fanout_encode_many(src_off, len, opcode, m, d_keys, k, d_wire, at, wire_off, true))
                return WSG_EINVAL;
            for (uint32_t i = 0; i < m; ++i)
                if (len[i] && !in_alloc(d_payload + src_off[i], len[i]))
                    return WSG_EINVAL;
        }
        hipStream_t s = as_stream(stream);
        const int t = timing_begin(c, s);
        if (int rc = fanout_many(c, s, d_payload, src_off, len, opcode, m, d_keys, k, mask, d_wire, wire_off))
            return rc;
        timing_end(c, s, t);
        return WSG_OK;
    } catch (...) {
        return WSG_ENOMEM;
    }
}
