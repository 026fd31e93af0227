// wsg_relay.hip — wsg_relay_validated: a round's received messages as
// unmasked server frames, one range of d_relay per room.  Plan kernels only;
// the payload moves through k_msg_gather (wsg_messages.hip), launched a second
// time over the relay's own piece records.
//
// The kernels run behind wsg_reply_validated's whole plan and read what it
// left: d_info, d_msgs (in the order of the frames that end the messages, so a
// stream's records are neighbours and their last frames ascend), the merged
// d_verdict and the message count (MsgPlan.tot[0]).  Of the assembly rule they
// read its name and, under WSG_ASSEMBLY_RFC, where a message of several frames
// is its data frames alone and a control frame is a message of its own, the
// frame that ends each frame's message (RfcPlan.eo).
//   k_relay_local          one lane per message: relayed or not (relay_op, the
//                          terminal cut), the frame's size (send_geom, mask 0);
//                          block-local sums of sizes and frames; the first and
//                          last record of every stream; inv[d_order[p]] = the lowest such p
//   k_relay_frames         one lane per frame: its message by bisection of the
//                          records' last frames; block-local sums of the data
//                          bytes and the pieces of the relayed frames
//   k_relay_blocks         those four over the block partials, a block each
//   k_relay_streams_local  one lane per position p: the permutation test, S of
//                          stream d_order[p], block-local sums of S; a lane per
//                          d_group_first entry: its rule
//   k_relay_streams_blocks those over the block partials; d_count[5..8), the
//                          latches, the gather's totals
//   k_relay_finalize       message lanes: d_relay_off, header and status
//                          prefix; frame lanes: piece records; a lane per
//                          group: d_group_relay
// Every sum is a scan, and the two atomicMin sites (inv in k_relay_local, the
// lowest offending position in k_relay_streams_local) keep a minimum: the
// outputs do not depend on the launch shape.
#include "wsg_msgplan.h"

namespace wsg {

namespace {

__device__ __forceinline__ uint32_t msg_last_frame(const wsg_msg* __restrict__ m)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(m);
    return uint32_t(w[2] >> 32) + uint32_t(w[3]) - 1;
}
__device__ __forceinline__ uint32_t msg_stream(const wsg_msg* __restrict__ m)
{
    return uint32_t(reinterpret_cast<const uint64_t*>(m)[2]);
}

// What message mr is relayed as (op 0: it is not): relay_op names its kind and
// the frame that ends it lies in front of its stream's terminal frame.
__device__ __forceinline__ ReplyOf relay_of(const ReplyRule& rule, const MsgRec& mr, uint32_t last, uint32_t ns,
                                            const uint64_t* __restrict__ verdict)
{
    ReplyOf a = reply_of(rule, mr.kind, mr.op, mr.len, mr.status);
    if (mr.stream >= ns || last >= verdict_frame(verdict[mr.stream]))
        a.op = 0;
    return a;
}

// Batch-wide values of the block-local scans, for an index in [0, count].
__device__ __forceinline__ uint64_t relay_before_msg(const RelayPlan& Q, uint64_t nmsg, uint64_t m)
{
    return m < nmsg ? Q.mex[m] + Q.bm_pre[m / BLOCK] : Q.tot[0];
}
__device__ __forceinline__ uint64_t data_before_frame(const RelayPlan& Q, uint32_t k)   // k < n
{
    return Q.fex[k] + Q.bw_pre[k / BLOCK];
}
__device__ __forceinline__ uint64_t relay_before_pos(const RelayPlan& Q, uint32_t ns, uint32_t p)
{
    return p < ns ? Q.pex[p] + Q.bs_pre[p / BLOCK] : Q.gtot[2];
}

// Where message m of stream j starts in d_relay: its room's bytes in front of
// the stream's position, then the stream's relayed messages in front of m.
__device__ __forceinline__ uint64_t relay_at(const RelayPlan& Q, const uint32_t* __restrict__ order, uint32_t ns,
                                             uint64_t nmsg, uint32_t j, uint64_t m)
{
    const uint32_t p = order ? Q.inv[j] : j;
    return relay_before_pos(Q, ns, p) + relay_before_msg(Q, nmsg, m) - relay_before_msg(Q, nmsg, Q.mfirst[j]);
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_relay_local(const wsg_msg* __restrict__ msgs,
                                                       const uint64_t* __restrict__ ptot, uint32_t ns,
                                                       const uint64_t* __restrict__ verdict, ReplyRule rule,
                                                       const uint32_t* __restrict__ order, RelayPlan Q)
{
    const uint64_t m = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint64_t nmsg = ptot[0];
    for (uint64_t p = m; order && p < ns; p += uint64_t(gridDim.x) * BLOCK) {
        const uint32_t j = order[p];
        if (j < ns)   // the lowest position of a stream named twice keeps it
            atomicMin(Q.inv + j, uint32_t(p));
    }
    uint64_t size = 0;
    if (m < nmsg) {
        const MsgRec mr = get_msg(msgs + m);
        size = reply_size(rule, relay_of(rule, mr, msg_last_frame(msgs + m), ns, verdict));
        if (mr.stream < ns) {
            if (m == 0 || msg_stream(msgs + m - 1) != mr.stream)
                Q.mfirst[mr.stream] = uint32_t(m);
            if (m + 1 == nmsg || msg_stream(msgs + m + 1) != mr.stream)
                Q.mend[mr.stream] = uint32_t(m + 1);
        }
    }
    uint64_t tb, tn;
    const uint64_t eb = block_scan_ex(size, OpAdd{}, &tb);
    block_scan_ex(uint64_t(size != 0), OpAdd{}, &tn);
    if (m < nmsg)
        Q.mex[m] = eb;
    if (threadIdx.x == 0) {
        Q.bm[blockIdx.x] = tb;
        Q.bn[blockIdx.x] = tn;
    }
}

// RFC: WSG_ASSEMBLY_RFC, where a frame's message is the one that ends at
// eo[i] (RfcPlan.eo: control frames delivered between two fragments have
// records of their own in front of the fragments' message), and the data
// offsets count data frames alone (a relayed control frame between two
// fragments is not a part of their message).  Under the reference rule a
// message is every frame from its first to its last.
template <bool RFC>
__global__ __launch_bounds__(BLOCK) void k_relay_frames(const wsg_recv_info* __restrict__ info, uint32_t n,
                                                        const wsg_msg* __restrict__ msgs,
                                                        const uint64_t* __restrict__ ptot, uint32_t ns,
                                                        const uint64_t* __restrict__ verdict, ReplyRule rule,
                                                        const uint32_t* __restrict__ eo, RelayPlan Q)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    const uint64_t nmsg = ptot[0];
    uint64_t moved = 0, data = 0;
    if (i64 < n) {
        const uint32_t e = RFC ? eo[i] : i;   // (UINT32_MAX: not delivered, and no record ends there)
        uint64_t a = 0, b = nmsg;             // the first record whose last frame is at or behind e
        while (a < b) {
            const uint64_t mid = a + (b - a) / 2;
            if (msg_last_frame(msgs + mid) < e)
                a = mid + 1;
            else
                b = mid;
        }
        uint32_t owner = UINT32_MAX;
        if (a < nmsg) {
            const MsgRec mr = get_msg(msgs + a);
            const uint32_t last = msg_last_frame(msgs + a);
            const wsg_recv_info r = info[i];
            const bool ctl = (r.opcode & 8u) != 0;
            const bool mine = RFC ? last == e : mr.first <= i;
            const ReplyOf ra = relay_of(rule, mr, last, ns, verdict);
            if (mine && ra.op && ra.len && r.len) {
                owner = uint32_t(a);
                moved = r.len;
                data = RFC && ctl ? 0 : r.len;
            }
        }
        Q.fmsg[i] = owner;
    }
    uint64_t tw, tp;
    const uint64_t ew = block_scan_ex(data, OpAdd{}, &tw);
    const uint64_t ep = block_scan_ex(msg_pieces_of(moved), OpAdd{}, &tp);
    if (i64 < n) {
        Q.fex[i] = ew;
        Q.fpc[i] = uint32_t(ep);
    }
    if (threadIdx.x == 0) {
        Q.bw[blockIdx.x] = tw;
        Q.bp[blockIdx.x] = tp;
    }
}

// Four blocks, a scan each (one block doing the four in turn took 43 us at
// 1 Mi frames, beside 5 to 25 us for each of the plan's other kernels).
__global__ __launch_bounds__(BLOCK) void k_relay_blocks(RelayPlan Q, uint32_t nb)
{
    const uint32_t which = blockIdx.x;   // 0: relay bytes, 1: relay frames, 2: pieces, 3: data bytes
    const uint64_t* in = which == 0 ? Q.bm : which == 1 ? Q.bn : which == 2 ? Q.bp : Q.bw;
    uint64_t* pre = which == 0 ? Q.bm_pre : which == 1 ? nullptr : which == 2 ? Q.bp_pre : Q.bw_pre;
    const uint64_t total = scan_partials(in, pre, nb, OpAdd{});
    if (threadIdx.x == 0 && which < 3)
        Q.tot[which] = total;
}

__global__ __launch_bounds__(BLOCK) void k_relay_streams_local(const uint64_t* __restrict__ ptot, uint32_t ns,
                                                               const uint32_t* __restrict__ order,
                                                               const uint32_t* __restrict__ group_first,
                                                               uint32_t ng, RelayPlan Q)
{
    const uint64_t p64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint64_t nmsg = ptot[0];
    // d_group_first's rule, entry g offending: keyed behind every position
    for (uint64_t g = p64; group_first && g <= ng; g += uint64_t(gridDim.x) * BLOCK) {
        const uint32_t v = group_first[g];
        if ((g == 0 && v != 0) || (g > 0 && v < group_first[g - 1]) || (g == ng && v != ns))
            atomicMin(reinterpret_cast<unsigned long long*>(Q.bad), static_cast<unsigned long long>(ns) + g);
    }
    uint64_t S = 0;
    if (p64 < ns) {
        const uint32_t p = uint32_t(p64);
        const uint32_t j = order ? order[p] : p;
        if (j < ns && (!order || Q.inv[j] == p))
            S = relay_before_msg(Q, nmsg, Q.mend[j]) - relay_before_msg(Q, nmsg, Q.mfirst[j]);
        else   // out of range, or a stream that a lower position names too
            atomicMin(reinterpret_cast<unsigned long long*>(Q.bad), static_cast<unsigned long long>(p));
    }
    uint64_t ts;
    const uint64_t es = block_scan_ex(S, OpAdd{}, &ts);
    if (p64 < ns)
        Q.pex[p64] = es;
    if (threadIdx.x == 0)
        Q.bs[blockIdx.x] = ts;
}

__global__ __launch_bounds__(BLOCK) void k_relay_streams_blocks(RelayPlan Q, uint32_t nbs, uint32_t n,
                                                                uint64_t relay_cap, uint64_t* __restrict__ count,
                                                                unsigned long long* err)
{
    const uint64_t cs = scan_partials(Q.bs, Q.bs_pre, nbs, OpAdd{});
    if (threadIdx.x == 0) {
        const uint64_t bad = Q.bad[0];
        const bool ok = bad == UINT64_MAX;
        const uint64_t bytes = ok ? cs : 0;
        count[5] = bytes;
        count[6] = ok ? Q.tot[1] : 0;
        count[7] = 0;
        Q.gtot[0] = ok;
        Q.gtot[1] = 0;
        Q.gtot[2] = bytes;                                    // k_msg_gather's view: bytes against the capacity
        Q.gtot[3] = ok && bytes <= relay_cap ? Q.tot[2] : 0;   // and the piece count
        // behind every frame error and the reply's capacity: the latch keeps the smallest
        if (!ok)
            latch(err, uint64_t(n) + 1 + bad, WSG_EINVAL);
        else if (bytes > relay_cap)
            latch(err, uint64_t(n) + 1, WSG_ENOMEM);
    }
}

__global__ __launch_bounds__(BLOCK) void k_relay_finalize(
    const wsg_recv_info* __restrict__ info, uint32_t n, const wsg_msg* __restrict__ msgs,
    const uint64_t* __restrict__ ptot, uint32_t ns, const uint64_t* __restrict__ verdict, ReplyRule rule,
    const uint32_t* __restrict__ order, const uint32_t* __restrict__ group_first, uint32_t ng, RelayPlan Q,
    uint8_t* __restrict__ relay, uint64_t relay_cap, uint64_t* __restrict__ relay_off,
    uint64_t* __restrict__ group_relay, MsgPiece* __restrict__ pieces, uint64_t pieces_cap)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    const uint64_t nmsg = ptot[0], total = Q.gtot[2];
    const bool ok = Q.gtot[0] != 0;
    // room g's bytes start where its first position's do (no table: one room of everyone)
    for (uint64_t g = i64; g <= ng; g += uint64_t(gridDim.x) * BLOCK) {
        const uint32_t p = group_first ? group_first[g] : (g == 0 ? 0u : ns);
        group_relay[g] = ok ? relay_before_pos(Q, ns, p) : 0;
    }
    if (i64 < nmsg) {
        const MsgRec mr = get_msg(msgs + i64);
        const ReplyOf a = relay_of(rule, mr, msg_last_frame(msgs + i64), ns, verdict);
        uint64_t at = UINT64_MAX;
        if (ok && a.op) {
            at = relay_at(Q, order, ns, nmsg, mr.stream, i64);
            const FrameRec R = make_rec(at, nullptr, a.len, 0u, a.status, a.op, false);
            const uint64_t head = R.hdr + R.prefix;
            if (total <= relay_cap && at <= relay_cap && head <= relay_cap - at) {
                const v4u h = frame_head(R);
                for (uint32_t t = 0; t < head; ++t)
                    relay[at + t] = uint8_t(lane_byte(h, t));
            }
        }
        relay_off[i64] = at;
    }
    uint64_t lo = 0, hi = 0, poff = 0, d0 = 0, plen = 0;
    uint32_t key = 0;
    if (i64 < n && ok) {
        const uint64_t before = uint64_t(Q.fpc[i]) + Q.bp_pre[i / BLOCK];
        const uint32_t m = Q.fmsg[i];
        if (m != UINT32_MAX) {   // (k_relay_frames' decision: relayed, with data, this frame a part of it)
            const wsg_recv_info r = info[i];
            const MsgRec mr = get_msg(msgs + m);
            const ReplyOf a = relay_of(rule, mr, msg_last_frame(msgs + m), ns, verdict);
            const FrameRec R = make_rec(relay_at(Q, order, ns, nmsg, mr.stream, m), nullptr, a.len, 0u, a.status,
                                        a.op, false);
            piece_range(before, before + msg_pieces_of(r.len), pieces_cap, lo, hi);
            // the frame's data offset in its message (a control frame of its own: 0)
            const uint64_t rel = mr.first < i && mr.first < n ? data_before_frame(Q, i) - data_before_frame(Q, mr.first)
                                                                : 0;
            // (inside the message unless stream_first is malformed: never a store outside the frame)
            if (rel <= a.len && r.len <= a.len - rel) {
                poff = r.payload_off;
                plen = r.len;
                d0 = R.pw + R.prefix + rel;
                key = r.key;   // the send key is 0: the receive key alone
            }
        }
    }
    // (a range whose frame gets no data keeps d0 = plen = 0: its pieces are empty)
    fill_pieces_wave(pieces, lo, hi, poff, d0, plen, key);
}

uint64_t relay_plan_layout(uint8_t* base, uint32_t n, uint32_t ns, RelayPlan* plan)
{
    // (at least one block each: the kernels that also serve the rooms run one block without a frame or a stream)
    const uint64_t nb = std::max<uint64_t>((uint64_t(n) + BLOCK - 1) / BLOCK, 1);
    const uint64_t nbs = std::max<uint64_t>((uint64_t(ns) + BLOCK - 1) / BLOCK, 1);
    Carve c{base, 16};
    RelayPlan Q;
    Q.mex = c.take<uint64_t>(n);
    Q.fex = c.take<uint64_t>(n);
    Q.pex = c.take<uint64_t>(ns);
    for (uint64_t** p : {&Q.bm, &Q.bm_pre, &Q.bn, &Q.bw, &Q.bw_pre, &Q.bp, &Q.bp_pre})
        *p = c.take<uint64_t>(nb);
    Q.bs = c.take<uint64_t>(nbs);
    Q.bs_pre = c.take<uint64_t>(nbs);
    Q.tot = c.take<uint64_t>(4);
    Q.gtot = c.take<uint64_t>(4);
    Q.bad = c.take<uint64_t>(1);
    Q.fpc = c.take<uint32_t>(n);
    Q.fmsg = c.take<uint32_t>(n);
    Q.mfirst = c.take<uint32_t>(ns);   // mfirst | mend | inv: one run, preset by two fills
    Q.mend = c.take<uint32_t>(ns);
    Q.inv = c.take<uint32_t>(ns);
    if (plan)
        *plan = Q;
    return c.at;
}

hipError_t launch_relay_plan(hipStream_t s, const Batch& b, const MsgOut& o, const wsg_proto_verdict* verdict,
                             const RelayArgs& relay, const RelayPlan& Q, const MsgScratch& x)
{
    const uint32_t n = b.n, n_streams = b.n_streams;
    const uint32_t nb = uint32_t((uint64_t(n) + BLOCK - 1) / BLOCK);
    const uint32_t nbs = uint32_t((uint64_t(n_streams) + BLOCK - 1) / BLOCK);
    const uint64_t* v = reinterpret_cast<const uint64_t*>(verdict);
    const uint64_t* ptot = x.plans.ref.tot;
    const ReplyRule rule = reply_rule(relay.relay_op, 0);   // a relay frame is unmasked (reply_size reads the mask)
    if (n_streams) {
        const uint64_t run = reinterpret_cast<uint8_t*>(Q.inv) - reinterpret_cast<uint8_t*>(Q.mfirst);
        if (hipError_t e = hipMemsetAsync(Q.mfirst, 0, run, s); e != hipSuccess)
            return e;
        if (hipError_t e = hipMemsetAsync(Q.inv, 0xFF, uint64_t(n_streams) * sizeof(uint32_t), s); e != hipSuccess)
            return e;
    }
    if (hipError_t e = hipMemsetAsync(Q.bad, 0xFF, sizeof(uint64_t), s); e != hipSuccess)
        return e;
    k_relay_local<<<(nb ? nb : 1u), BLOCK, 0, s>>>(o.msgs, ptot, n_streams, v, rule, relay.order, Q);
    if (n) {
        if (x.plans.assembly == WSG_ASSEMBLY_RFC)
            k_relay_frames<true><<<nb, BLOCK, 0, s>>>(o.info, n, o.msgs, ptot, n_streams, v, rule, x.plans.rfc.eo, Q);
        else
            k_relay_frames<false><<<nb, BLOCK, 0, s>>>(o.info, n, o.msgs, ptot, n_streams, v, rule, nullptr, Q);
    }
    k_relay_blocks<<<4, BLOCK, 0, s>>>(Q, nb);
    k_relay_streams_local<<<(nbs ? nbs : 1u), BLOCK, 0, s>>>(ptot, n_streams, relay.order, relay.group_first,
                                                              relay.n_groups, Q);
    k_relay_streams_blocks<<<1, BLOCK, 0, s>>>(Q, nbs, n, relay.relay_cap, o.count, x.err);
    k_relay_finalize<<<(nb ? nb : 1u), BLOCK, 0, s>>>(o.info, n, o.msgs, ptot, n_streams, v, rule, relay.order,
                                                         relay.group_first, relay.n_groups, Q, relay.relay,
                                                         relay.relay_cap, relay.relay_off, relay.group_relay, x.pieces,
                                                         x.pieces_cap);
    return hipGetLastError();
}

} // namespace wsg
