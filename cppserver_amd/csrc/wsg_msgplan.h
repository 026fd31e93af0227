// wsg_msgplan.h — what the two message plans (wsg_messages.hip: the
// reference's assembly rule; wsg_assembly.hip: RFC 6455 5.4) share on the
// device: the gather's piece records, the reply a message is answered with,
// the reply prefix and the verdict word of the checked replies.  Internal
// linkage, as wsg_device.h.
#pragma once

#include "wsg_device.h"

namespace wsg {
namespace {

__device__ __forceinline__ uint64_t msg_pieces_of(uint64_t bytes)
{
    return bytes ? (bytes + PIECE_ALIGN - 1 + PIECE - 1) / PIECE : 0;
}

__device__ __forceinline__ void put_piece(MsgPiece* p, uint64_t poff, uint64_t d0, uint64_t len, uint32_t key,
                                          uint32_t k)
{
    static_assert(sizeof(MsgPiece) == 32 && offsetof(MsgPiece, len) == 16 && offsetof(MsgPiece, k) == 28, "MsgPiece");
    v4u* w = reinterpret_cast<v4u*>(p);
    w[0] = v4u{uint32_t(poff), uint32_t(poff >> 32), uint32_t(d0), uint32_t(d0 >> 32)};
    w[1] = v4u{uint32_t(len), uint32_t(len >> 32), key, k};
}

// pieces[t] for t in [lo, hi) of every lane's frame (fill_tiles_wave's
// scheme: a frame of many pieces is written by the whole wave).
__device__ __forceinline__ void fill_pieces_wave(MsgPiece* pieces, uint64_t lo, uint64_t hi, uint64_t poff,
                                                 uint64_t d0, uint64_t len, uint32_t key)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr uint64_t kShort = 4;   // ranges up to this many pieces: the lane stores its own
    if (hi > lo && hi - lo <= kShort)
        for (uint64_t t = lo; t < hi; ++t)
            put_piece(pieces + t, poff, d0, len, key, uint32_t(t - lo));
    uint64_t pending = __ballot(hi > lo + kShort);
    while (pending) {
        const int j = __builtin_ctzll(pending);
        pending &= pending - 1;
        const uint64_t a = lane_bcast(lo, j), b = lane_bcast(hi, j);
        const uint64_t pj = lane_bcast(poff, j), dj = lane_bcast(d0, j), lj = lane_bcast(len, j);
        const uint32_t kj = __builtin_amdgcn_readlane(key, j);
        for (uint64_t t = a + lane; t < b; t += 64)
            put_piece(pieces + t, pj, dj, lj, kj, uint32_t(t - a));
    }
}

// What message r is answered with: the first header byte (0: nothing), the
// data length and the status of the PrepareSendFrame call.
struct ReplyOf {
    uint8_t op;
    uint64_t len;
    int32_t status;
};

__device__ __forceinline__ ReplyOf reply_of(const ReplyRule& rule, uint32_t kind, uint32_t opcode, uint64_t len,
                                            int32_t status)
{
    const uint8_t v = kind >= 1 && kind <= 4 ? rule.op[kind] : uint8_t(0);
    ReplyOf r;
    r.op = v == WSG_REPLY_SAME ? uint8_t(WSG_FIN | opcode) : v;
    r.len = kind == WSG_CB_CLOSE ? 0 : len;   // a close reply carries the status and no data
    r.status = kind == WSG_CB_CLOSE ? status : 0;
    return r;
}

__device__ __forceinline__ uint64_t reply_size(const ReplyRule& rule, const ReplyOf& r)
{
    if (!r.op)
        return 0;
    const SendGeom g = send_geom(r.op, rule.mask != 0, r.len, r.status);
    return g.hdr + g.body;
}

// Reply bytes of the FIN frames before frame k, for k in [0, n].
__device__ __forceinline__ uint64_t reply_before(const MsgPlan& P, uint32_t n, uint32_t k)
{
    return k < n ? P.rex[k] + P.brep_pre[k / BLOCK] : P.rtot[2];
}

// ---- wsg_reply_checked: a stream's effective verdict, as the reply kernels read it
// (one little-endian word: code, pad, status, the terminal frame on top; all
// 0xFF: none, and then no frame index equals or exceeds its frame).
__device__ __forceinline__ uint32_t verdict_frame(uint64_t v) { return uint32_t(v >> 32); }

// The close frame a verdict is answered with: PrepareSendFrame(WSG_FIN | WSG_CLOSE,
// mask, NULL, 0, status); 1005 never goes on the wire (RFC 6455 7.4.1).
__device__ __forceinline__ int32_t close_status(uint64_t v)
{
    const int32_t s = int32_t((v >> 16) & 0xFFFFu);
    return s == 1005 ? 1000 : s;
}

__device__ __forceinline__ uint64_t close_size(const ReplyRule& rule, uint64_t v)
{
    const SendGeom g = send_geom(uint8_t(WSG_FIN | WSG_CLOSE), rule.mask != 0, 0, close_status(v));
    return g.hdr + g.body;
}

} // namespace
} // namespace wsg
