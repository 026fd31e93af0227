// wsg_messages.hip — message assembly and replies on the device
// (wsg_decode_messages, wsg_reply_messages, wsg_reply_checked): the plan
// kernels, k_msg_gather and their launchers.
#include "wsg_msgplan.h"

namespace wsg {

// ===========================================================================
// Message assembly: wsg_decode_messages
// ===========================================================================
//
// The second half of PrepareReceiveFrame (ws.cpp:399-452) over a batch whose
// frames are grouped into streams: every FIN frame ends a message made of the
// unmasked payloads of its stream's frames since the previous FIN frame, and
// the messages are packed back to back into one buffer.
//
// Plan pass, one lane per frame (BLOCK frames per block, block partials
// scanned by one block in between):
//   k_msg_scan_local   header parse (d_info, error latch), the frame's stream,
//                      and three block-local scans: FIN frames before i (sum),
//                      last frame <= i that heads a stream or names an opcode
//                      (max: the sticky _ws_opcode), last FIN frame < i (max:
//                      where i's message began)
//   k_msg_scan_blocks  the three over the block partials; d_count[0]
//   k_msg_bytes_local  a frame is delivered when its stream has a FIN frame
//                      at or after it; block-local sums of delivered bytes
//                      (the frame's offset in d_msg) and of pieces
//   k_msg_bytes_blocks those over the block partials; d_count[1]; WSG_ENOMEM
//   k_msg_finalize     FIN lanes write their wsg_msg; the gather's piece records
//   k_msg_state        one lane per stream: consumed, _ws_opcode
// Gather pass (k_msg_gather), the mirror of k_encode_mask: a piece is at most
// PIECE bytes of ONE frame's payload cut at absolute 16-byte chunks of the
// DESTINATION (rows on 128-byte lines), one wave per piece, so the key, the
// key phase (byte index in the frame's payload mod 4) and the source shift
// are uniform over it.  Full chunks: one aligned 16-B nontemporal load per
// lane, the second block of the 32-byte window taken from the next lane's
// registers, v_alignbyte funnel, XOR, 16-B nontemporal store.  The two chunks a frame shares with its
// neighbours in d_msg: each frame stores only its own bytes (neighbours run
// in other waves).

// k_msg_gather's source loads (tools/msgbench.py, one box, C2 / C3 in
// fragments, us): a chunk's second 16-B block is the next lane's first, so
// it comes from that lane's registers and every block is loaded once, with
// the nontemporal hint: 90.8 / 731.  Loaded a second time instead (as
// k_encode_mask does): 94.4 / 769 with plain first loads, 110.7 / 832 with
// nontemporal ones (the second read then misses); shuffled but plain loads
// 91.3 / 778.
#ifndef WSG_MSG_SHFL
#define WSG_MSG_SHFL 1    // the second block from the next lane's registers (0: a second load)
#endif
#ifndef WSG_MSG_NT_LO
#define WSG_MSG_NT_LO 1   // nontemporal loads of a chunk's first source block
#endif
#ifndef WSG_MSG_NT_HI
#define WSG_MSG_NT_HI 1   // ... and of a second block that is loaded
#endif

namespace {

// Batch-wide values of the plan's block-local scans, for k in [0, n].
__device__ __forceinline__ uint64_t fins_before(const MsgPlan& P, uint32_t n, uint32_t k)
{
    return k < n ? uint64_t(P.finx[k]) + P.bfin_pre[k / BLOCK] : P.tot[0];
}
__device__ __forceinline__ uint32_t last_fin_before(const MsgPlan& P, uint32_t n, uint32_t k)   // + 1; 0: none
{
    return k < n ? max(P.qx[k], P.bq_pre[k / BLOCK]) : uint32_t(P.tot[1]);
}
__device__ __forceinline__ uint64_t dst_of(const MsgPlan& P, uint32_t k)   // k < n
{
    return P.dst[k] + P.bbytes_pre[k / BLOCK];
}
__device__ __forceinline__ uint64_t pieces_before(const MsgPlan& P, uint32_t n, uint32_t k)
{
    return k < n ? uint64_t(P.pstart[k]) + P.bpc_pre[k / BLOCK] : P.tot[3];
}
// _ws_opcode after frame i of stream j (ws.cpp:326): the last non-zero
// opcode of the stream up to i, else the stream's seed.
__device__ __forceinline__ uint32_t sticky_opcode(const MsgPlan& P, const wsg_recv_info* __restrict__ info,
                                                  const wsg_stream_state* state, uint32_t i, uint32_t j)
{
    const uint32_t pv = max(P.pinc[i], P.bp_pre[i / BLOCK]);
    const uint32_t op = pv ? info[pv - 1].opcode : 0u;
    return op ? op : state[j].opcode;
}

// The message that FIN frame i ends (ws.cpp:411-452), as the wsg_msg fields.
__device__ __forceinline__ MsgRec msg_at_fin(const uint8_t* __restrict__ wire, const wsg_recv_info* __restrict__ info,
                                             uint32_t n, const uint32_t* __restrict__ sf,
                                             const wsg_stream_state* __restrict__ state, const MsgPlan& P, uint32_t i,
                                             uint64_t frame_len)
{
    const uint32_t j = P.sidx[i];
    const uint32_t ff = min(max(last_fin_before(P, n, i), sf[j]), i);   // the message's first frame
    const uint64_t base = dst_of(P, ff), end = dst_of(P, i) + frame_len;
    const uint32_t op = sticky_opcode(P, info, state, i, j);
    uint64_t off = base, len = end - base;
    uint32_t kind = 0;
    int32_t status = 0;
    if (op == WSG_TEXT || op == WSG_BINARY) {
        kind = WSG_CB_RECEIVED;
    } else if (op == WSG_PING) {
        kind = WSG_CB_PING;
    } else if (op == WSG_PONG) {
        kind = WSG_CB_PONG;
    } else if (op == WSG_CLOSE) {
        kind = WSG_CB_CLOSE;
        status = 1000;
        if (len >= 2) {   // ws.cpp:435-439: the buffer's first two bytes, wherever their frames are
            uint32_t sb[2];
            for (uint32_t t = 0; t < 2; ++t) {
                const uint64_t x = base + t;
                uint32_t a = ff, b = i + 1;   // last k in [ff, i] with dst_of(k) <= x holds byte x
                while (b - a > 1) {
                    const uint32_t mid = a + (b - a) / 2;
                    if (dst_of(P, mid) <= x)
                        a = mid;
                    else
                        b = mid;
                }
                const uint64_t o = x - dst_of(P, a);
                // (o < len unless stream_first is malformed: never a read past the payload)
                sb[t] = o < info[a].len ? uint32_t(wire[info[a].payload_off + o]) ^ key_byte(info[a].key, o) : 0u;
            }
            status = int32_t((sb[0] << 8) | sb[1]);
            off += 2;
            len -= 2;
        }
    }
    return MsgRec{off, len, j, ff, kind, op, status};
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_msg_scan_local(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                          const uint64_t* __restrict__ fs, uint32_t n,
                                                          const uint32_t* __restrict__ sf, uint32_t ns,
                                                          wsg_recv_info* __restrict__ info, MsgPlan P,
                                                          unsigned long long* err)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint32_t fin = 0, pv = 0;
    if (i64 < n) {
        wsg_recv_info r;
        const int e = frame_parse(wire, wire_len, fs[i], i + 1 < n ? fs[i + 1] : wire_len, r);
        if (e != 0)
            latch(err, i, e);
        store_info(info + i, r);
        const uint32_t j = stream_of(sf, ns, i);
        P.sidx[i] = j;
        fin = r.fin;
        pv = (r.opcode != 0 || sf[j] == i) ? i + 1 : 0;
    }
    uint32_t tf, tp, tq;
    const uint32_t ef = block_scan_ex(fin, OpAdd{}, &tf);
    const uint32_t ep = block_scan_ex(pv, OpMax{}, &tp);
    const uint32_t eq = block_scan_ex(fin ? i + 1 : 0u, OpMax{}, &tq);
    if (i64 < n) {
        P.finx[i] = ef;
        P.pinc[i] = max(ep, pv);
        P.qx[i] = eq;
    }
    if (threadIdx.x == 0) {
        P.bfin[blockIdx.x] = tf;
        P.bp[blockIdx.x] = tp;
        P.bq[blockIdx.x] = tq;
    }
}

__global__ __launch_bounds__(BLOCK) void k_msg_scan_blocks(MsgPlan P, uint32_t nb, uint64_t* __restrict__ count)
{
    const uint32_t cf = scan_partials(P.bfin, P.bfin_pre, nb, OpAdd{});
    scan_partials(P.bp, P.bp_pre, nb, OpMax{});
    const uint32_t cq = scan_partials(P.bq, P.bq_pre, nb, OpMax{});
    if (threadIdx.x == 0) {
        P.tot[0] = cf;
        P.tot[1] = cq;
        count[0] = cf;
    }
}

__global__ __launch_bounds__(BLOCK) void k_msg_bytes_local(const wsg_recv_info* __restrict__ info, uint32_t n,
                                                           const uint32_t* __restrict__ sf, MsgPlan P)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t dl = 0;
    if (i64 < n) {
        const uint32_t end = min(sf[P.sidx[i] + 1], n);
        if (fins_before(P, n, end) > fins_before(P, n, i))   // a FIN frame in [i, end): not in the tail
            dl = info[i].len;
    }
    uint64_t tb, tp;
    const uint64_t eb = block_scan_ex(dl, OpAdd{}, &tb);
    const uint64_t ep = block_scan_ex(msg_pieces_of(dl), OpAdd{}, &tp);
    if (i64 < n) {
        P.dst[i] = eb;
        P.pstart[i] = uint32_t(ep);
    }
    if (threadIdx.x == 0) {
        P.bbytes[blockIdx.x] = tb;
        P.bpc[blockIdx.x] = tp;
    }
}

__global__ __launch_bounds__(BLOCK) void k_msg_bytes_blocks(MsgPlan P, uint32_t nb, uint32_t n, uint64_t msg_cap,
                                                            uint64_t* __restrict__ count, unsigned long long* err)
{
    const uint64_t cb = scan_partials(P.bbytes, P.bbytes_pre, nb, OpAdd{});
    const uint64_t cp = scan_partials(P.bpc, P.bpc_pre, nb, OpAdd{});
    if (threadIdx.x == 0) {
        P.tot[2] = cb;
        P.tot[3] = cp;
        count[1] = cb;
        if (cb > msg_cap)   // behind every frame error: the latch keeps the smallest
            latch(err, n, WSG_ENOMEM);
    }
}

__global__ __launch_bounds__(BLOCK) void k_msg_finalize(const uint8_t* __restrict__ wire,
                                                        const wsg_recv_info* __restrict__ info, uint32_t n,
                                                        const uint32_t* __restrict__ sf,
                                                        const wsg_stream_state* __restrict__ state, MsgPlan P,
                                                        wsg_msg* __restrict__ msgs,
                                                        MsgPiece* __restrict__ pieces, uint64_t pieces_cap)
{
    if (uint64_t(blockIdx.x) * BLOCK + (threadIdx.x & ~63u) >= n)
        return;   // whole wave past the last frame
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t lo = 0, hi = 0, poff = 0, d0 = 0, plen = 0;
    uint32_t key = 0;
    if (i64 < n) {
        piece_range(pieces_before(P, n, i), pieces_before(P, n, i + 1), pieces_cap, lo, hi);
        const wsg_recv_info r = info[i];
        poff = r.payload_off;
        plen = r.len;
        key = r.key;
        d0 = dst_of(P, i);
        if (r.fin)
            put_msg(msgs + fins_before(P, n, i), msg_at_fin(wire, info, n, sf, state, P, i, r.len), i);
    }
    fill_pieces_wave(pieces, lo, hi, poff, d0, plen, key);
}

__global__ __launch_bounds__(BLOCK) void k_msg_state(const wsg_recv_info* __restrict__ info, uint32_t n,
                                                     const uint32_t* __restrict__ sf, uint32_t ns,
                                                     wsg_stream_state* state, MsgPlan P)
{
    static_assert(sizeof(wsg_stream_state) == 8 && offsetof(wsg_stream_state, opcode) == 4, "wsg_stream_state layout");
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    const uint32_t j = uint32_t(j64);
    const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
    uint32_t consumed = 0, op = state[j].opcode;
    if (fins_before(P, n, end) > fins_before(P, n, start)) {
        const uint32_t last = last_fin_before(P, n, end);   // + 1: in (start, end]
        if (last > start && last <= end) {
            consumed = last - start;
            op = sticky_opcode(P, info, state, last - 1, j);
        }
    }
    *reinterpret_cast<uint64_t*>(state + j) = uint64_t(consumed) | (uint64_t(op & 0xFFu) << 32);
}

// wsg_reply_checked: d_state[j].consumed alone, behind k_msg_scan_blocks: the
// protocol judge reads it, and k_msg_state, which writes the same value
// beside the opcode, has to stay behind the reply kernels (they read the
// opcode's seed).
__global__ __launch_bounds__(BLOCK) void k_msg_consumed(uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns,
                                                        wsg_stream_state* state, MsgPlan P)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    const uint32_t j = uint32_t(j64);
    const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
    uint32_t consumed = 0;
    if (fins_before(P, n, end) > fins_before(P, n, start)) {
        const uint32_t last = last_fin_before(P, n, end);   // + 1: in (start, end]
        if (last > start && last <= end)
            consumed = last - start;
    }
    state[j].consumed = consumed;
}

// ---- replies (wsg_reply_messages) -------------------------------------------
// The plan above up to k_msg_bytes_blocks, then, one lane per frame again:
//   k_reply_local     FIN lanes write their wsg_msg and size the reply frame
//                     (send_geom); block-local sums of the reply sizes.  The
//                     sum over the FIN frames before frame i is the reply
//                     offset of the message frame i belongs to, FIN or not.
//   k_reply_blocks    those over the block partials; d_count[2..3]; the
//                     capacity latch; the gather's totals (P.rtot)
//   k_reply_finalize  FIN lanes: d_reply_off, header and status prefix (byte
//                     stores, frame_head's bytes); every lane: its frame's
//                     piece records with the reply wire as destination and
//                     the receive key XOR the send key at the destination's
//                     phase; a lane per stream: d_stream_reply
// and k_msg_gather over those records: every payload byte is read once from
// the received wire and written once, re-keyed, into its reply frame.
// wsg_reply_checked runs the CHECKED instantiations of the three behind the
// protocol kernels (wsg_proto.hip): every frame lane reads its stream's
// effective verdict through P.sidx, a reply is sized only in front of the
// terminal frame t, lane t sizes and writes the stream's close frame, and the
// per-stream lanes write d_close_off.  The close frame belongs to frame t as a
// reply belongs to its FIN frame, so one scan places both.

// CHECKED (wsg_reply_checked): frame i sizes its reply only in front of its
// stream's terminal frame t, and the close frame's size when i == t; the
// block sum of reply frames carries the close frames in its upper half too.
// (Kernel templates, not a shared body: the rule stays a kernel argument,
// whose bytes are indexed where they lie; a copy of it would live in scratch.)
template <bool CHECKED>
__global__ __launch_bounds__(BLOCK) void k_reply_local(const uint8_t* __restrict__ wire,
                                                       const wsg_recv_info* __restrict__ info, uint32_t n,
                                                       const uint32_t* __restrict__ sf,
                                                       const wsg_stream_state* __restrict__ state, MsgPlan P,
                                                       ReplyRule rule, wsg_msg* __restrict__ msgs,
                                                       const uint64_t* __restrict__ verdict)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t size = 0, frames = 0;
    if (CHECKED) {
        if (i64 < n) {
            const uint64_t v = verdict[P.sidx[i]];
            if (info[i].fin) {   // every record is written, answered or not
                const MsgRec m = msg_at_fin(wire, info, n, sf, state, P, i, info[i].len);
                put_msg(msgs + fins_before(P, n, i), m, i);
                if (i < verdict_frame(v))
                    size = reply_size(rule, reply_of(rule, m.kind, m.op, m.len, m.status));
            }
            frames = size != 0;
            if (i == verdict_frame(v)) {   // (and then size == 0)
                size = close_size(rule, v);
                frames = 1 | (1ull << 32);
            }
        }
    } else {
        if (i64 < n && info[i].fin) {
            const MsgRec m = msg_at_fin(wire, info, n, sf, state, P, i, info[i].len);
            put_msg(msgs + fins_before(P, n, i), m, i);
            size = reply_size(rule, reply_of(rule, m.kind, m.op, m.len, m.status));
        }
        frames = size != 0;
    }
    uint64_t tb, tn;
    const uint64_t eb = block_scan_ex(size, OpAdd{}, &tb);
    block_scan_ex(frames, OpAdd{}, &tn);
    if (i64 < n)
        P.rex[i] = eb;
    if (threadIdx.x == 0) {
        P.brep[blockIdx.x] = tb;
        P.brn[blockIdx.x] = tn;
    }
}

template <bool CHECKED>
__global__ __launch_bounds__(BLOCK) void k_reply_blocks(MsgPlan P, uint32_t nb, uint32_t n, uint64_t reply_cap,
                                             uint64_t* __restrict__ count, unsigned long long* err)
{
    const uint64_t cb = scan_partials(P.brep, P.brep_pre, nb, OpAdd{});
    const uint64_t cn = scan_partials<uint64_t>(P.brn, nullptr, nb, OpAdd{});
    if (threadIdx.x == 0) {
        P.rtot[2] = cb;         // k_msg_gather's view of the totals: bytes against the capacity,
        P.rtot[3] = P.tot[3];   // and the piece count
        count[2] = cb;
        if (CHECKED) {          // (frames <= n < 2^32: the halves do not meet)
            count[3] = uint32_t(cn);
            count[4] = cn >> 32;
        } else {
            count[3] = cn;
        }
        if (cb > reply_cap)   // behind every frame error: the latch keeps the smallest
            latch(err, n, WSG_ENOMEM);
    }
}

template <bool CHECKED>
__global__ __launch_bounds__(BLOCK) void k_reply_finalize(
    const wsg_recv_info* __restrict__ info, uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns, MsgPlan P,
    ReplyRule rule, const uint32_t* __restrict__ send_key, const wsg_msg* __restrict__ msgs,
    uint8_t* __restrict__ reply, uint64_t reply_cap, uint64_t* __restrict__ reply_off,
    uint64_t* __restrict__ stream_reply, MsgPiece* __restrict__ pieces, uint64_t pieces_cap,
    const uint64_t* __restrict__ verdict, uint64_t* __restrict__ close_off)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    const uint64_t total = P.rtot[2], nmsg = P.tot[0];
    // connection j's replies start where its first message's does
    for (uint64_t j = i64; j <= ns; j += uint64_t(gridDim.x) * BLOCK) {
        stream_reply[j] = reply_before(P, n, min(sf[j], n));
        if (CHECKED && j < ns) {   // its close frame belongs to the terminal frame, which holds no reply
            const uint32_t t = verdict_frame(verdict[j]);
            close_off[j] = t < n && P.sidx[t] == uint32_t(j) ? reply_before(P, n, t) : UINT64_MAX;
        }
    }
    if (i64 == 0)
        reply_off[nmsg] = total;
    uint64_t lo = 0, hi = 0, poff = 0, d0 = 0, plen = 0;
    uint32_t key = 0;
    if (i64 < n) {
        piece_range(pieces_before(P, n, i), pieces_before(P, n, i + 1), pieces_cap, lo, hi);
        const wsg_recv_info r = info[i];
        const uint64_t m = fins_before(P, n, i);
        if (CHECKED) {
            const uint32_t j = P.sidx[i];
            const uint64_t v = verdict[j];
            if (i == verdict_frame(v) && total <= reply_cap) {   // the terminal frame's lane: the close frame
                const uint64_t at = reply_before(P, n, i);
                const FrameRec R = make_rec(at, nullptr, 0, send_key ? send_key[j] : 0u, close_status(v),
                                            uint8_t(WSG_FIN | WSG_CLOSE), rule.mask != 0);
                const v4u h = frame_head(R);
                for (uint32_t t = 0; t < R.hdr + R.prefix; ++t)
                    reply[at + t] = uint8_t(lane_byte(h, t));
            }
        }
        if ((r.fin || hi > lo) && m < nmsg) {   // frame i belongs to message m
            const MsgRec mr = get_msg(msgs + m);
            ReplyOf a = reply_of(rule, mr.kind, mr.op, mr.len, mr.status);
            if (CHECKED) {   // k_reply_local's decision, taken at the message's FIN frame
                const uint32_t nframes = uint32_t(reinterpret_cast<const uint64_t*>(msgs + m)[3]);
                if (mr.first + nframes - 1 >= verdict_frame(verdict[mr.stream]))
                    a.op = 0;
            }
            const uint64_t at = reply_before(P, n, i);
            const uint32_t skey = send_key ? send_key[mr.stream] : 0u;
            if (r.fin)
                reply_off[m] = at;
            if (a.op) {
                const FrameRec R = make_rec(at, nullptr, a.len, skey, a.status, a.op, rule.mask != 0);
                if (r.fin && total <= reply_cap) {
                    const v4u h = frame_head(R);
                    for (uint32_t t = 0; t < R.hdr + R.prefix; ++t)
                        reply[at + t] = uint8_t(lane_byte(h, t));
                }
                // data byte dst_of(i) - mr.off of the message: c bytes into the reply's payload
                // (inside the message unless stream_first is malformed: never a store outside the frame)
                const uint64_t rel = dst_of(P, i) - mr.off;
                if (a.len && dst_of(P, i) >= mr.off && rel <= a.len && r.len <= a.len - rel) {
                    const uint64_t c = R.prefix + rel;
                    poff = r.payload_off;
                    plen = r.len;
                    d0 = R.pw + c;
                    key = r.key ^ key_rot(skey, uint32_t(c));
                }
            }
        }
    }
    // (a frame whose message gets no data keeps d0 = plen = 0: its pieces are empty)
    fill_pieces_wave(pieces, lo, hi, poff, d0, plen, key);
}

__global__ __launch_bounds__(BLOCK) void k_msg_gather(const uint8_t* __restrict__ wire,
                                                      const uint64_t* __restrict__ tot,
                                                      const MsgPiece* __restrict__ piece_recs, uint64_t pieces_cap,
                                                      uint8_t* __restrict__ msg, uint64_t msg_cap)
{
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t q0 = uint64_t(blockIdx.x) * (BLOCK / 64) + wave_id();
    if (tot[2] > msg_cap)
        return;   // WSG_ENOMEM latched by k_msg_bytes_blocks: no byte of msg
    const uint64_t pieces = min(tot[3], pieces_cap);
    for (uint64_t q = q0; q < pieces; q += waves) {
        // the record as dwords (wave-uniform: one scalar load, as load_desc)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(piece_recs + q);
        const uint64_t poff = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
        const uint64_t d0 = uint64_t(w[2]) | (uint64_t(w[3]) << 32);
        const uint64_t len = uint64_t(w[4]) | (uint64_t(w[5]) << 32);
        const uint32_t key = w[6];
        const uint64_t k = w[7];
        const uint64_t end = d0 + len;
        const uint64_t lo = (d0 & ~(PIECE_ALIGN - 1)) + k * PIECE;
        if (lo >= end || end > msg_cap)
            continue;   // piece counts are an upper bound
        const uint64_t hi = min(lo + PIECE, end);
        // source of msg byte p: src + (p - d0), as pointer arithmetic on the
        // wire argument (global_* loads)
        const uint8_t* src = wire + poff;
        const uint32_t s = uint32_t((reinterpret_cast<uintptr_t>(src) + (lo - d0)) & 15u);
        const uint32_t kw = key_rot(key, uint32_t(lo - d0));   // phase: byte index in the payload (mod 4 also when lo < d0)
        v4u a[EU], b[EU];
        uint32_t full = 0;
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            const bool f = p < hi && p >= d0 && p + CHUNK <= end;
            full |= uint32_t(f) << u;
            const uint8_t* a0 = src + (int64_t(p - d0) - int64_t(s));
            a[u] = f ? (WSG_MSG_NT_LO ? ld16nt(a0) : ld16(a0)) : v4u{0, 0, 0, 0};
        }
#if !WSG_MSG_SHFL
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            const uint8_t* a0 = src + (int64_t(p - d0) - int64_t(s));
            b[u] = ((full >> u) & 1u) && s ? (WSG_MSG_NT_HI ? ld16nt(a0 + CHUNK) : ld16(a0 + CHUNK)) : v4u{0, 0, 0, 0};
        }
#else
        // bit u: the lane after this one in the piece (lane 0 of the next row
        // for lane 63) loaded the block after a[u] as its own first block
        const uint32_t nfull = lane == 63 ? uint32_t(__builtin_amdgcn_readlane(full, 0)) >> 1
                                          : uint32_t(__shfl_down(full, 1, 64));
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            const uint8_t* a0 = src + (int64_t(p - d0) - int64_t(s));
            b[u] = ((full >> u) & 1u) && s && !((nfull >> u) & 1u)
                       ? (WSG_MSG_NT_HI ? ld16nt(a0 + CHUNK) : ld16(a0 + CHUNK))
                       : v4u{0, 0, 0, 0};
        }
        if (s) {
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                v4u nx;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t first = u + 1 < EU ? uint32_t(__builtin_amdgcn_readlane(a[u + 1 < EU ? u + 1 : u][c], 0)) : 0u;
                    const uint32_t down = uint32_t(__shfl_down(a[u][c], 1, 64));
                    nx[c] = lane == 63 ? first : down;
                }
                if ((nfull >> u) & 1u)
                    b[u] = nx;
            }
        }
#endif
        // the full chunks first, in a straight line: with the edge chunks'
        // loads and byte stores between them every store waited for the one
        // before it (stores count in vmcnt on gfx9)
#pragma unroll
        for (int u = 0; u < EU; ++u)
            a[u] = (s ? funnel(a[u], b[u], s) : a[u]) ^ kw;
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            if ((full >> u) & 1u)
                st16nt(msg + p, a[u]);
        }
        // the (at most two) chunks shared with a neighbour frame: this
        // frame's bytes only; wave-uniform test, most pieces have none
        const bool head_edge = lo <= d0 && (d0 & (CHUNK - 1)) != 0;
        const bool tail_edge = hi == end && (end & (CHUNK - 1)) != 0;
        if (!head_edge && !tail_edge)
            continue;
#pragma unroll 1
        for (uint32_t u = 0; u < uint32_t(EU); ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            if (((full >> u) & 1u) || p >= hi || p + CHUNK <= d0)
                continue;
            const v4u v = fan_window(src, len, int64_t(p) - int64_t(d0)) ^ kw;
            const uint32_t o_lo = p < d0 ? uint32_t(d0 - p) : 0u;
            const uint32_t o_hi = end - p < CHUNK ? uint32_t(end - p) : uint32_t(CHUNK);
            uint32_t* m32 = reinterpret_cast<uint32_t*>(msg + p);
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const uint32_t b0 = 4 * c, b1 = b0 + 4;
                if (b0 >= o_lo && b1 <= o_hi) {
                    m32[c] = v[c];
                } else {
                    for (uint32_t t = max(b0, o_lo); t < min(b1, o_hi); ++t)
                        msg[p + t] = uint8_t(v[c] >> (8 * (t - b0)));
                }
            }
        }
    }
}

uint64_t msg_plan_layout(uint8_t* base, uint32_t n, MsgPlan* plan)
{
    const uint64_t nb = (uint64_t(n) + BLOCK - 1) / BLOCK;
    Carve c{base, 16};
    MsgPlan P;
    P.dst = c.take<uint64_t>(n);
    P.bbytes = c.take<uint64_t>(nb);
    P.bbytes_pre = c.take<uint64_t>(nb);
    P.bpc = c.take<uint64_t>(nb);
    P.bpc_pre = c.take<uint64_t>(nb);
    P.tot = c.take<uint64_t>(4);
    P.finx = c.take<uint32_t>(n);
    P.pinc = c.take<uint32_t>(n);
    P.qx = c.take<uint32_t>(n);
    P.sidx = c.take<uint32_t>(n);
    P.pstart = c.take<uint32_t>(n);
    P.bfin = c.take<uint32_t>(nb);
    P.bfin_pre = c.take<uint32_t>(nb);
    P.bp = c.take<uint32_t>(nb);
    P.bp_pre = c.take<uint32_t>(nb);
    P.bq = c.take<uint32_t>(nb);
    P.bq_pre = c.take<uint32_t>(nb);
    P.rex = c.take<uint64_t>(n);
    P.brep = c.take<uint64_t>(nb);
    P.brep_pre = c.take<uint64_t>(nb);
    P.brn = c.take<uint64_t>(nb);
    P.rtot = c.take<uint64_t>(4);
    if (plan)
        *plan = P;
    return c.at;
}

// What the two plans share: the scans up to k_msg_bytes_blocks (under
// WSG_ASSEMBLY_RFC: launch_rfc_scans, which reads seed[j].ahead) and then
// finish(nb), or, for no frame (no message, every stream unchanged with
// nothing consumed), the totals and count_words of d_count zeroed; k_msg_state
// (launch_rfc_state) behind either when `state` is given.
template <class Finish>
static hipError_t launch_plan(hipStream_t s, const Batch& b, wsg_stream_state* state, const wsg_stream_state* seed,
                              uint64_t msg_cap, const MsgOut& o, uint32_t count_words, const MsgScratch& x,
                              Finish finish)
{
    const MsgPlan& plan = x.plans.ref;
    const bool rfc = x.plans.assembly == WSG_ASSEMBLY_RFC;
    const uint32_t nb = uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK);
    hipError_t re = hipSuccess;   // of the other source's launchers (each has taken its launch's error)
    if (b.n == 0) {
        if (hipError_t e = hipMemsetAsync(plan.tot, 0, 4 * sizeof(uint64_t), s); e != hipSuccess)
            return e;
        if (hipError_t e = hipMemsetAsync(o.count, 0, count_words * sizeof(uint64_t), s); e != hipSuccess)
            return e;
    } else if (rfc) {
        re = launch_rfc_scans(s, b, seed, msg_cap, o, x);
        finish(nb);
    } else {
        k_msg_scan_local<<<nb, BLOCK, 0, s>>>(b.wire, b.wire_len, b.fs, b.n, b.stream_first, b.n_streams, o.info, plan,
                                              x.err);
        k_msg_scan_blocks<<<1, BLOCK, 0, s>>>(plan, nb, o.count);
        k_msg_bytes_local<<<nb, BLOCK, 0, s>>>(o.info, b.n, b.stream_first, plan);
        k_msg_bytes_blocks<<<1, BLOCK, 0, s>>>(plan, nb, b.n, msg_cap, o.count, x.err);
        finish(nb);
    }
    if (b.n_streams && state) {
        if (rfc) {
            if (hipError_t e = launch_rfc_state(s, b.n, b.stream_first, b.n_streams, state, x.plans.rfc, false);
                re == hipSuccess)
                re = e;
        } else {
            k_msg_state<<<(b.n_streams + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(o.info, b.n, b.stream_first, b.n_streams,
                                                                             state, plan);
        }
    }
    const hipError_t e = hipGetLastError();
    return re != hipSuccess ? re : e;
}

// k_msg_finalize, or its part under WSG_ASSEMBLY_RFC.
static hipError_t launch_finalize(hipStream_t s, uint32_t nb, const Batch& b, const wsg_stream_state* state,
                                  const MsgOut& o, const MsgScratch& x)
{
    if (x.plans.assembly == WSG_ASSEMBLY_RFC)
        return launch_rfc_finalize(s, b, o, x);
    k_msg_finalize<<<nb, BLOCK, 0, s>>>(b.wire, o.info, b.n, b.stream_first, state, x.plans.ref, o.msgs, x.pieces,
                                        x.pieces_cap);
    return hipGetLastError();
}

hipError_t launch_msg_plan(hipStream_t s, const Batch& b, wsg_stream_state* state, const wsg_stream_state* seed,
                           uint64_t msg_cap, const MsgOut& o, const MsgScratch& x)
{
    hipError_t fe = hipSuccess;
    const hipError_t e = launch_plan(s, b, state, seed, msg_cap, o, 2, x,
                                     [&](uint32_t nb) { fe = launch_finalize(s, nb, b, seed, o, x); });
    return fe != hipSuccess ? fe : e;
}

hipError_t launch_gather(hipStream_t s, int grid, const uint8_t* wire, const uint64_t* tot, const MsgPiece* pieces,
                         uint64_t pieces_cap, uint8_t* dst, uint64_t dst_cap)
{
    k_msg_gather<<<grid, BLOCK, 0, s>>>(wire, tot, pieces, pieces_cap, dst, dst_cap);
    return hipGetLastError();
}

// A batch of no frame has no reply either: the totals, d_reply_off[0] and
// d_stream_reply zeroed, and no stream closed (r.close_off, when checked).
static hipError_t reply_of_none(hipStream_t s, uint32_t n_streams, const MsgPlan& plan, const ReplyOut& r)
{
    if (hipError_t e = hipMemsetAsync(plan.rtot, 0, 4 * sizeof(uint64_t), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(r.reply_off, 0, sizeof(uint64_t), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(r.stream_reply, 0, (uint64_t(n_streams) + 1) * sizeof(uint64_t), s);
        e != hipSuccess)
        return e;
    if (r.close_off && n_streams)
        return hipMemsetAsync(r.close_off, 0xFF, uint64_t(n_streams) * sizeof(uint64_t), s);
    return hipSuccess;
}

// The reply kernels behind the message plan's scans (n > 0); v: d_verdict as
// words when CHECKED, null otherwise.
template <bool CHECKED>
static hipError_t launch_reply_kernels(hipStream_t s, uint32_t nb, const Batch& b, const wsg_stream_state* state,
                                       const ReplyOut& r, const MsgOut& o, const MsgScratch& x, const uint64_t* v)
{
    const MsgPlan& plan = x.plans.ref;
    const ReplyRule rule = reply_rule(r.reply_op, r.mask);
    if (x.plans.assembly == WSG_ASSEMBLY_RFC) {
        const hipError_t e = launch_rfc_reply_local(s, CHECKED, b, o, x, rule, v);
        k_reply_blocks<CHECKED><<<1, BLOCK, 0, s>>>(plan, nb, b.n, r.reply_cap, o.count, x.err);
        const hipError_t f = launch_rfc_reply_finalize(s, CHECKED, b, o, x, r, rule, v);
        return e != hipSuccess ? e : f;
    }
    k_reply_local<CHECKED><<<nb, BLOCK, 0, s>>>(b.wire, o.info, b.n, b.stream_first, state, plan, rule, o.msgs, v);
    k_reply_blocks<CHECKED><<<1, BLOCK, 0, s>>>(plan, nb, b.n, r.reply_cap, o.count, x.err);
    k_reply_finalize<CHECKED><<<nb, BLOCK, 0, s>>>(o.info, b.n, b.stream_first, b.n_streams, plan, rule, r.send_key,
                                                   o.msgs, r.reply, r.reply_cap, r.reply_off, r.stream_reply, x.pieces,
                                                   x.pieces_cap, v, r.close_off);
    return hipSuccess;   // (launch_plan takes the launches' error)
}

hipError_t launch_reply_plan(hipStream_t s, const Batch& b, wsg_stream_state* state, const ReplyOut& r,
                             const MsgOut& o, const MsgScratch& x)
{
    if (b.n == 0)
        if (hipError_t e = reply_of_none(s, b.n_streams, x.plans.ref, r); e != hipSuccess)
            return e;
    hipError_t fe = hipSuccess;
    // (no d_msg: its size, d_count[1], meets no capacity)
    const hipError_t e = launch_plan(s, b, state, state, UINT64_MAX, o, 4, x, [&](uint32_t nb) {
        fe = launch_reply_kernels<false>(s, nb, b, state, r, o, x, nullptr);
    });
    return fe != hipSuccess ? fe : e;
}

hipError_t launch_reply_checked_plan(hipStream_t s, int stream_grid, const Batch& b, wsg_stream_state* state,
                                     const ProtoOps& p, const ProtoPlan& pplan, const ReplyOut& r, const MsgOut& o,
                                     const MsgScratch& x, const Utf8Inside* utf8)
{
    hipError_t pe = hipSuccess;   // of the other sources' launchers (each has taken its launch's error)
    const auto keep = [&pe](hipError_t e) {
        if (pe == hipSuccess)
            pe = e;
    };
    if (b.n == 0) {   // no reply, no close frame, nothing judged: the seeds, and d_proto as it came
        if (hipError_t e = reply_of_none(s, b.n_streams, x.plans.ref, r); e != hipSuccess)
            return e;
        keep(launch_proto_scan(s, b, o.info, p, pplan));
        keep(launch_proto_finish(s, stream_grid, b, state, p, pplan));
        if (utf8)   // no record: d_utf8_result's seed is its value
            keep(launch_utf8_init(s, 1, o.msgs, o.count, 0, utf8->valid, utf8->result));
    }
    const hipError_t e = launch_plan(s, b, state, state, UINT64_MAX, o, 5, x, [&](uint32_t nb) {
        // (n > 0, so n_streams > 0: the caller checks)
        if (x.plans.assembly == WSG_ASSEMBLY_RFC)
            keep(launch_rfc_state(s, b.n, b.stream_first, b.n_streams, state, x.plans.rfc, true));
        else
            k_msg_consumed<<<(b.n_streams + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(b.n, b.stream_first, b.n_streams, state,
                                                                                x.plans.ref);
        keep(launch_proto_scan(s, b, o.info, p, pplan));
        keep(launch_proto_judge(s, b, o.info, state, p, pplan));
        const wsg_proto_verdict* also = p.also;
        if (utf8) {
            // wsg_reply_validated: the dense piece records (the reply's replace them below), the
            // check from the wire over them, its verdicts beside the caller's
            keep(launch_finalize(s, nb, b, state, o, x));
            keep(launch_utf8_init(s, utf8->rec_grid, o.msgs, o.count, b.n, utf8->valid, utf8->result));
            if (utf8->which)
                keep(launch_utf8_wire(s, utf8->wire_grid, b, o, x, utf8->which, utf8->valid));
            keep(launch_utf8_count(s, utf8->rec_grid, o.msgs, o.count, b.n, UINT64_MAX, utf8->which, utf8->valid,
                                   utf8->result));
            keep(launch_utf8_verdicts_over(s, stream_grid, b, also, o, *utf8));
            also = reinterpret_cast<const wsg_proto_verdict*>(utf8->also);
        }
        if (also)
            keep(launch_proto_merge(s, stream_grid, b.n, b.stream_first, b.n_streams, also, p.verdict));
        keep(launch_proto_finish(s, stream_grid, b, state, p, pplan));
        keep(launch_reply_kernels<true>(s, nb, b, state, r, o, x, reinterpret_cast<const uint64_t*>(p.verdict)));
    });
    return pe != hipSuccess ? pe : e;
}

} // namespace wsg
