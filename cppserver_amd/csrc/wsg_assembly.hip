// wsg_assembly.hip — WSG_ASSEMBLY_RFC: the message plan under RFC 6455 5.4
// (wsg_set_assembly).  Control frames between the fragments of a message are
// messages of their own, delivered in the call they arrive in; a data message
// is its data frames alone.  Plan kernels only: the piece records they write
// are in dense order, so k_msg_gather and k_utf8_wire (wsg_messages.hip,
// wsg_utf8.hip) run over them as they run over the reference rule's.
//
// The sequential walk this restates (layout.message_plan, assembly=RFC) has one
// state per stream: the open run's first frame, whether a run was delivered
// yet, and the count of control frames an earlier call delivered ahead of the
// open run (wsg_stream_state.ahead).  Here every frame finds its run from scans
// (RfcPlan, wsg_internal.h), one lane per frame:
//   k_rfc_scan_local   header parse (d_info, error latch), the frame's stream
//                      and class; block-local counts of the classes before i,
//                      last DF frame < i, last stream head <= i, last D frame
//                      <= i that names an opcode
//   k_rfc_scan_blocks  those over the block partials
//   k_rfc_bytes_local  the frame's run by bisection of the counts (the first D
//                      frame behind the last DF frame or head; the next DF
//                      frame, if no head lies between), whether it is delivered
//                      (a data frame: its run ends in this call; a control
//                      frame: by its rank in the open run, see deliver_control);
//                      block-local sums of delivered bytes and pieces, of
//                      those of control frames, and of message-ending frames
//   k_rfc_bytes_blocks those over the block partials; d_count[0..1]; WSG_ENOMEM
//   k_rfc_finalize     message-ending lanes write their wsg_msg; every
//                      delivered lane its piece records
//   k_rfc_state        one lane per stream: consumed, ahead
// and k_rfc_reply_local / k_rfc_reply_finalize in the places of the reference
// rule's, around its k_reply_blocks.
//
// Dense order.  For a run [ff, e] the delivered control frames in [ff, e) come
// first, then the run's data frames; with A(k), C(k) the delivered bytes and
// delivered control bytes before frame k:
//   data frame i     A(i) + C(e) - C(i)
//   control frame c  A(ff) + C(c) - C(ff)          (no run open: ff = c)
// and the same with piece counts for the index of the frame's first record.
#include "wsg_msgplan.h"

namespace wsg {

namespace {

constexpr uint32_t AHEAD_CAP = 65535;   // wsg_stream_state.ahead is 16 bits wide
enum : int { F_D = 0, F_DF = 1, F_C = 2, F_H = 3 };

struct FrameClass {
    bool d, df, c;
};

__device__ __forceinline__ FrameClass class_of(uint32_t opcode, uint32_t fin, uint32_t error)
{
    const bool ok = error == 0, ctl = (opcode & 8u) != 0;
    return FrameClass{ok && !ctl, ok && !ctl && fin != 0, ok && ctl && fin != 0};
}

// (opcode, fin, error) of a d_info record, from its words (store_info's layout).
__device__ __forceinline__ FrameClass class_of(const wsg_recv_info* __restrict__ info, uint32_t i, uint64_t* len,
                                               uint32_t* opcode)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(info + i);
    const uint64_t w2 = w[2];
    *len = w[1];
    *opcode = uint32_t(w2 >> 32) & 0xFFu;
    return class_of(*opcode, uint32_t(w2 >> 40) & 0xFFu, uint32_t(w[3] >> 8) & 0xFFu);
}

// Frames of class F before frame k, for k in [0, n].
template <int F>
__device__ __forceinline__ uint32_t class_before(const RfcPlan& R, uint32_t n, uint32_t k)
{
    if (k >= n)
        return uint32_t(R.tot[F]);
    const uint32_t* pre = F == F_D ? R.bD_pre : F == F_DF ? R.bDF_pre : F == F_C ? R.bC_pre : R.bH_pre;
    return ((R.cnt[k] >> (8 * F)) & 0xFFu) + pre[k / BLOCK];
}

// The first frame of class F in [x, hi), hi <= n; hi: there is none.
template <int F>
__device__ __forceinline__ uint32_t first_of(const RfcPlan& R, uint32_t n, uint32_t x, uint32_t hi)
{
    if (x >= hi)
        return hi;
    const uint32_t p0 = class_before<F>(R, n, x);
    if (class_before<F>(R, n, hi) == p0)
        return hi;
    uint32_t a = x, b = hi;   // class_before(a) == p0 < class_before(b)
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (class_before<F>(R, n, mid) > p0)
            b = mid;
        else
            a = mid;
    }
    return b - 1;
}

__device__ __forceinline__ uint32_t last_df_before(const RfcPlan& R, uint32_t n, uint32_t k)   // + 1; 0: none
{
    return k < n ? max(R.qd[k], R.bqd_pre[k / BLOCK]) : uint32_t(R.tot[4]);
}

// Where the run that frame i < n lies in may begin: behind the last DF frame
// before i, at the last stream head at or before i.
__device__ __forceinline__ uint32_t run_floor(const RfcPlan& R, uint32_t n, uint32_t i, bool* first_run)
{
    const uint32_t df = last_df_before(R, n, i), hq = max(R.hq[i], R.bhq_pre[i / BLOCK]);
    const uint32_t head = hq ? hq - 1 : 0;
    *first_run = df <= head;   // no run of the stream was delivered in front of this one
    return max(df, head);
}

// The DF frame that ends the run of frame i (of class D or C; i itself when it
// is one); n: the run stays open in this call.
__device__ __forceinline__ uint32_t run_end(const RfcPlan& R, uint32_t n, uint32_t i)
{
    const uint32_t e = first_of<F_DF>(R, n, i, n);
    return e < n && class_before<F_H>(R, n, e + 1) == class_before<F_H>(R, n, i + 1) ? e : n;
}

// Batch-wide values of k_rfc_bytes_local's sums, k < n.
__device__ __forceinline__ uint64_t bytes_before(const RfcPlan& R, uint32_t k) { return R.ab[k] + R.bab_pre[k / BLOCK]; }
__device__ __forceinline__ uint64_t ctl_bytes_before(const RfcPlan& R, uint32_t k)
{
    return R.cb[k] + R.bcb_pre[k / BLOCK];
}
__device__ __forceinline__ uint64_t pieces_packed_before(const RfcPlan& R, uint32_t k)
{
    return R.pc[k] + R.bpc_pre[k / BLOCK];
}
__device__ __forceinline__ uint32_t enders_before(const RfcPlan& R, uint32_t k) { return R.ex[k] + R.bex_pre[k / BLOCK]; }

// Delivered frame i's place in the dense order: its payload's offset and the
// index of its first piece record.
struct Dense {
    uint64_t d0, p0;
};
__device__ __forceinline__ Dense dense_of(const RfcPlan& R, uint32_t i, bool control)
{
    // control: bytes before the run, control bytes of the run before i;
    // data: every delivered byte before i, control bytes of the run behind i
    const uint32_t a = control ? R.ff[i] : i, c0 = control ? R.ff[i] : i, c1 = control ? i : R.eo[i];
    const uint64_t pa = pieces_packed_before(R, a), p0 = pieces_packed_before(R, c0),
                   p1 = pieces_packed_before(R, c1);
    return Dense{bytes_before(R, a) + ctl_bytes_before(R, c1) - ctl_bytes_before(R, c0),
                 uint64_t(uint32_t(pa)) + (p1 >> 32) - (p0 >> 32)};
}

// The message that frame i ends (R.eo[i] == i).
__device__ __forceinline__ MsgRec rfc_msg_at(const uint8_t* __restrict__ wire, const wsg_recv_info* __restrict__ info,
                                             const uint32_t* __restrict__ sidx, const RfcPlan& R, uint32_t i)
{
    const wsg_recv_info r = info[i];
    const uint32_t ff = R.ff[i], j = sidx[i];
    if (r.opcode & 8u) {   // a control frame: a message of its own
        uint64_t off = dense_of(R, i, true).d0, len = r.len;
        const uint32_t op = r.opcode;
        uint32_t kind = op == WSG_PING ? WSG_CB_PING : op == WSG_PONG ? WSG_CB_PONG : op == WSG_CLOSE ? WSG_CB_CLOSE : 0u;
        int32_t status = 0;
        if (op == WSG_CLOSE) {
            status = 1000;
            if (len >= 2) {   // ws.cpp:435-439
                const uint32_t b0 = uint32_t(wire[r.payload_off]) ^ key_byte(r.key, 0);
                const uint32_t b1 = uint32_t(wire[r.payload_off + 1]) ^ key_byte(r.key, 1);
                status = int32_t((b0 << 8) | b1);
                off += 2;
                len -= 2;
            }
        }
        return MsgRec{off, len, j, i, kind, op, status};
    }
    // the run [ff, i]: its data frames' bytes behind the control frames delivered inside it
    const uint64_t ctl = ctl_bytes_before(R, i) - ctl_bytes_before(R, ff);
    const uint64_t base = bytes_before(R, ff);
    const uint32_t pv = max(R.pop[i], R.bpop_pre[i / BLOCK]);
    const uint32_t op = pv > ff ? info[pv - 1].opcode : 0u;
    const uint32_t kind = op == WSG_TEXT || op == WSG_BINARY ? WSG_CB_RECEIVED : 0u;
    return MsgRec{base + ctl, bytes_before(R, i) + r.len - base - ctl, j, ff, kind, op, 0};
}

// What a stream [start, end) leaves open: its consumed frames and, when a run
// is open, the FIN control frames behind the run's first frame.
__device__ __forceinline__ uint32_t stream_tail(const RfcPlan& R, uint32_t n, uint32_t start, uint32_t end,
                                                uint32_t* ahead)
{
    *ahead = 0;
    if (end <= start)
        return 0;
    const uint32_t f = first_of<F_D>(R, n, max(last_df_before(R, n, end), start), end);
    if (f < end)
        *ahead = min(class_before<F_C>(R, n, end) - class_before<F_C>(R, n, f), AHEAD_CAP);
    return f - start;
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_rfc_scan_local(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                          const uint64_t* __restrict__ fs, uint32_t n,
                                                          const uint32_t* __restrict__ sf, uint32_t ns,
                                                          wsg_recv_info* __restrict__ info,
                                                          uint32_t* __restrict__ sidx, RfcPlan R,
                                                          unsigned long long* err)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t add = 0;   // the four classes, 16 bits each (a block's total is at most BLOCK)
    uint32_t qd = 0, hq = 0, pop = 0;
    if (i64 < n) {
        wsg_recv_info r;
        const int e = frame_parse(wire, wire_len, fs[i], i + 1 < n ? fs[i + 1] : wire_len, r);
        if (e != 0)
            latch(err, i, e);
        store_info(info + i, r);
        const uint32_t j = stream_of(sf, ns, i);
        sidx[i] = j;
        const FrameClass c = class_of(r.opcode, r.fin, uint32_t(e != 0));
        const bool head = sf[j] == i;
        add = uint64_t(c.d) | uint64_t(c.df) << 16 | uint64_t(c.c) << 32 | uint64_t(head) << 48;
        qd = c.df ? i + 1 : 0;
        hq = head ? i + 1 : 0;
        pop = c.d && r.opcode ? i + 1 : 0;
    }
    uint64_t ta;
    uint32_t tq, th, tp;
    const uint64_t ea = block_scan_ex(add, OpAdd{}, &ta);
    const uint32_t eq = block_scan_ex(qd, OpMax{}, &tq);
    const uint32_t eh = block_scan_ex(hq, OpMax{}, &th);
    const uint32_t ep = block_scan_ex(pop, OpMax{}, &tp);
    if (i64 < n) {   // (the counts before a frame of the block: at most BLOCK - 1)
        R.cnt[i] = uint32_t(ea & 0xFFu) | uint32_t((ea >> 16) & 0xFFu) << 8 | uint32_t((ea >> 32) & 0xFFu) << 16 |
                   uint32_t((ea >> 48) & 0xFFu) << 24;
        R.qd[i] = eq;
        R.hq[i] = max(eh, hq);
        R.pop[i] = max(ep, pop);
    }
    if (threadIdx.x == 0) {
        R.bD[blockIdx.x] = uint32_t(ta & 0xFFFFu);
        R.bDF[blockIdx.x] = uint32_t((ta >> 16) & 0xFFFFu);
        R.bC[blockIdx.x] = uint32_t((ta >> 32) & 0xFFFFu);
        R.bH[blockIdx.x] = uint32_t(ta >> 48);
        R.bqd[blockIdx.x] = tq;
        R.bhq[blockIdx.x] = th;
        R.bpop[blockIdx.x] = tp;
    }
}

__global__ __launch_bounds__(BLOCK) void k_rfc_scan_blocks(RfcPlan R, uint32_t nb)
{
    const uint32_t cd = scan_partials(R.bD, R.bD_pre, nb, OpAdd{});
    const uint32_t cf = scan_partials(R.bDF, R.bDF_pre, nb, OpAdd{});
    const uint32_t cc = scan_partials(R.bC, R.bC_pre, nb, OpAdd{});
    const uint32_t ch = scan_partials(R.bH, R.bH_pre, nb, OpAdd{});
    const uint32_t cq = scan_partials(R.bqd, R.bqd_pre, nb, OpMax{});
    scan_partials(R.bhq, R.bhq_pre, nb, OpMax{});
    scan_partials(R.bpop, R.bpop_pre, nb, OpMax{});
    if (threadIdx.x == 0) {
        R.tot[0] = cd;
        R.tot[1] = cf;
        R.tot[2] = cc;
        R.tot[3] = ch;
        R.tot[4] = cq;
    }
}

// A FIN control frame i with run [f, ...) open (f < i), of rank `rank` among
// such frames since f: an earlier call delivered the first state.ahead of the
// stream's first run; the 16-bit count cannot tell the ones past AHEAD_CAP
// apart, so those wait for the call that holds the run's FIN frame.
__device__ __forceinline__ bool deliver_control(const RfcPlan& R, uint32_t n, uint32_t i, uint32_t rank,
                                                bool first_run, uint32_t ahead)
{
    if (first_run && rank < ahead)
        return false;
    return rank < AHEAD_CAP || run_end(R, n, i) < n;
}

__global__ __launch_bounds__(BLOCK) void k_rfc_bytes_local(const wsg_recv_info* __restrict__ info, uint32_t n,
                                                           const wsg_stream_state* __restrict__ state,
                                                           const uint32_t* __restrict__ sidx, RfcPlan R)
{
    static_assert(sizeof(wsg_stream_state) == 8 && offsetof(wsg_stream_state, ahead) == 6, "wsg_stream_state layout");
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t dl = 0, cl = 0;
    uint32_t ender = 0;
    if (i64 < n) {
        uint64_t len;
        uint32_t opcode;
        const FrameClass c = class_of(info, i, &len, &opcode);
        uint32_t ff = i, eo = UINT32_MAX;
        if (c.d) {
            const uint32_t e = c.df ? i : run_end(R, n, i);
            if (e < n) {
                dl = len;
                eo = e;
                if (c.df) {   // (a D frame lies in [floor, i]: i itself)
                    bool first_run;
                    ender = 1;
                    ff = first_of<F_D>(R, n, run_floor(R, n, i, &first_run), i + 1);
                }
            }
        } else if (c.c) {
            bool first_run;
            const uint32_t f = first_of<F_D>(R, n, run_floor(R, n, i, &first_run), i);
            bool deliver = true;
            if (f < i) {   // a run is open
                ff = f;
                deliver = deliver_control(R, n, i, class_before<F_C>(R, n, i) - class_before<F_C>(R, n, f), first_run,
                                          reinterpret_cast<const uint16_t*>(state + sidx[i])[3]);   // .ahead
            }
            if (deliver) {
                dl = cl = len;
                eo = i;
                ender = 1;
            }
        }
        R.ff[i] = ff;
        R.eo[i] = eo;
    }
    uint64_t tb, tc, tp;
    uint32_t te;
    const uint64_t eb = block_scan_ex(dl, OpAdd{}, &tb);
    const uint64_t ec = block_scan_ex(cl, OpAdd{}, &tc);
    const uint64_t ep = block_scan_ex(msg_pieces_of(dl) | msg_pieces_of(cl) << 32, OpAdd{}, &tp);
    const uint32_t ee = block_scan_ex(ender, OpAdd{}, &te);
    if (i64 < n) {
        R.ab[i] = eb;
        R.cb[i] = ec;
        R.pc[i] = ep;
        R.ex[i] = ee;
    }
    if (threadIdx.x == 0) {
        R.bab[blockIdx.x] = tb;
        R.bcb[blockIdx.x] = tc;
        R.bpc[blockIdx.x] = tp;
        R.bex[blockIdx.x] = te;
    }
}

// (the pieces of a batch fit 32 bits: the host refuses a larger bound)
__global__ __launch_bounds__(BLOCK) void k_rfc_bytes_blocks(uint64_t* __restrict__ tot, RfcPlan R, uint32_t nb,
                                                            uint32_t n, uint64_t msg_cap,
                                                            uint64_t* __restrict__ count, unsigned long long* err)
{
    const uint64_t cb = scan_partials(R.bab, R.bab_pre, nb, OpAdd{});
    scan_partials(R.bcb, R.bcb_pre, nb, OpAdd{});
    const uint64_t cp = scan_partials(R.bpc, R.bpc_pre, nb, OpAdd{});
    const uint32_t ce = scan_partials(R.bex, R.bex_pre, nb, OpAdd{});
    if (threadIdx.x == 0) {
        tot[0] = ce;
        tot[1] = R.tot[4];
        tot[2] = cb;
        tot[3] = uint32_t(cp);
        count[0] = ce;
        count[1] = cb;
        if (cb > msg_cap)   // behind every frame error: the latch keeps the smallest
            latch(err, n, WSG_ENOMEM);
    }
}

__global__ __launch_bounds__(BLOCK) void k_rfc_finalize(const uint8_t* __restrict__ wire,
                                                        const wsg_recv_info* __restrict__ info, uint32_t n,
                                                        const uint32_t* __restrict__ sidx, RfcPlan R,
                                                        wsg_msg* __restrict__ msgs, MsgPiece* __restrict__ pieces,
                                                        uint64_t pieces_cap)
{
    if (uint64_t(blockIdx.x) * BLOCK + (threadIdx.x & ~63u) >= n)
        return;   // whole wave past the last frame
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t lo = 0, hi = 0, poff = 0, d0 = 0, plen = 0;
    uint32_t key = 0;
    if (i64 < n && R.eo[i] != UINT32_MAX) {
        const wsg_recv_info r = info[i];
        const Dense at = dense_of(R, i, (r.opcode & 8u) != 0);
        piece_range(at.p0, at.p0 + msg_pieces_of(r.len), pieces_cap, lo, hi);
        poff = r.payload_off;
        plen = r.len;
        key = r.key;
        d0 = at.d0;
        if (R.eo[i] == i)
            put_msg(msgs + enders_before(R, i), rfc_msg_at(wire, info, sidx, R, i), i);
    }
    fill_pieces_wave(pieces, lo, hi, poff, d0, plen, key);
}

// CONSUMED_ONLY (wsg_reply_checked): d_state[j].consumed alone, ahead of the
// protocol judge, which reads it; the whole record behind the reply kernels.
template <bool CONSUMED_ONLY>
__global__ __launch_bounds__(BLOCK) void k_rfc_state(uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns,
                                                     wsg_stream_state* state, RfcPlan R)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    const uint32_t j = uint32_t(j64);
    const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
    uint32_t ahead;
    const uint32_t consumed = stream_tail(R, n, start, end, &ahead);   // (no frame: no read of the plan)
    if (CONSUMED_ONLY)
        state[j].consumed = consumed;
    else
        *reinterpret_cast<uint64_t*>(state + j) = uint64_t(consumed) | (uint64_t(ahead) << 48);
}

// ---- replies ------------------------------------------------------------------
// k_reply_local and k_reply_finalize (wsg_messages.hip) with "FIN frame" read
// as "frame that ends a delivered message": a reply belongs to that frame, and
// a data frame's pieces take their reply offset at their run's FIN frame.

template <bool CHECKED>
__global__ __launch_bounds__(BLOCK) void k_rfc_reply_local(const uint8_t* __restrict__ wire,
                                                           const wsg_recv_info* __restrict__ info, uint32_t n,
                                                           MsgPlan P, RfcPlan R, ReplyRule rule,
                                                           wsg_msg* __restrict__ msgs,
                                                           const uint64_t* __restrict__ verdict)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    uint64_t size = 0, frames = 0;
    if (i64 < n) {
        const uint64_t v = CHECKED ? verdict[P.sidx[i]] : ~0ull;
        if (R.eo[i] == i) {   // every record is written, answered or not
            const MsgRec m = rfc_msg_at(wire, info, P.sidx, R, i);
            put_msg(msgs + enders_before(R, i), m, i);
            if (i < verdict_frame(v))
                size = reply_size(rule, reply_of(rule, m.kind, m.op, m.len, m.status));
        }
        frames = size != 0;
        if (CHECKED && i == verdict_frame(v)) {   // (and then size == 0)
            size = close_size(rule, v);
            frames = 1 | (1ull << 32);
        }
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
__global__ __launch_bounds__(BLOCK) void k_rfc_reply_finalize(
    const wsg_recv_info* __restrict__ info, uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns, MsgPlan P,
    RfcPlan R, ReplyRule rule, const uint32_t* __restrict__ send_key, const wsg_msg* __restrict__ msgs,
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
        if (CHECKED) {
            const uint32_t j = P.sidx[i];
            const uint64_t v = verdict[j];
            if (i == verdict_frame(v) && total <= reply_cap) {   // the terminal frame's lane: the close frame
                const uint64_t at = reply_before(P, n, i);
                const FrameRec C = make_rec(at, nullptr, 0, send_key ? send_key[j] : 0u, close_status(v),
                                            uint8_t(WSG_FIN | WSG_CLOSE), rule.mask != 0);
                const v4u h = frame_head(C);
                for (uint32_t t = 0; t < C.hdr + C.prefix; ++t)
                    reply[at + t] = uint8_t(lane_byte(h, t));
            }
        }
        const uint32_t e = R.eo[i];   // the frame that ends frame i's message
        const uint64_t m = e != UINT32_MAX ? enders_before(R, e) : nmsg;
        if (m < nmsg) {
            const wsg_recv_info r = info[i];
            const Dense dense = dense_of(R, i, (r.opcode & 8u) != 0);
            piece_range(dense.p0, dense.p0 + msg_pieces_of(r.len), pieces_cap, lo, hi);
            const MsgRec mr = get_msg(msgs + m);
            ReplyOf a = reply_of(rule, mr.kind, mr.op, mr.len, mr.status);
            if (CHECKED && e >= verdict_frame(verdict[mr.stream]))   // k_rfc_reply_local's decision, taken at frame e
                a.op = 0;
            const uint64_t at = reply_before(P, n, e);
            const uint32_t skey = send_key ? send_key[mr.stream] : 0u;
            if (e == i)
                reply_off[m] = at;
            if (a.op) {
                const FrameRec F = make_rec(at, nullptr, a.len, skey, a.status, a.op, rule.mask != 0);
                if (e == i && total <= reply_cap) {
                    const v4u h = frame_head(F);
                    for (uint32_t t = 0; t < F.hdr + F.prefix; ++t)
                        reply[at + t] = uint8_t(lane_byte(h, t));
                }
                // data byte dense.d0 - mr.off of the message: c bytes into the reply's payload
                // (a close message's data starts behind its status: no byte of the frame is one)
                const uint64_t rel = dense.d0 - mr.off;
                if (a.len && dense.d0 >= mr.off && rel <= a.len && r.len <= a.len - rel) {
                    const uint64_t c = F.prefix + rel;
                    poff = r.payload_off;
                    plen = r.len;
                    d0 = F.pw + c;
                    key = r.key ^ key_rot(skey, uint32_t(c));
                }
            }
        }
    }
    // (a frame whose message gets no data keeps d0 = plen = 0: its pieces are empty)
    fill_pieces_wave(pieces, lo, hi, poff, d0, plen, key);
}

uint64_t rfc_plan_layout(uint8_t* base, uint32_t n, RfcPlan* plan)
{
    const uint64_t nb = (uint64_t(n) + BLOCK - 1) / BLOCK;
    Carve c{base, 16};
    RfcPlan R;
    R.ab = c.take<uint64_t>(n);
    R.cb = c.take<uint64_t>(n);
    R.pc = c.take<uint64_t>(n);
    for (uint64_t** p : {&R.bab, &R.bab_pre, &R.bcb, &R.bcb_pre, &R.bpc, &R.bpc_pre})
        *p = c.take<uint64_t>(nb);
    R.tot = c.take<uint64_t>(5);
    for (uint32_t** p : {&R.cnt, &R.qd, &R.hq, &R.pop, &R.ex, &R.ff, &R.eo})
        *p = c.take<uint32_t>(n);
    for (uint32_t** p : {&R.bD, &R.bD_pre, &R.bDF, &R.bDF_pre, &R.bC, &R.bC_pre, &R.bH, &R.bH_pre, &R.bqd, &R.bqd_pre,
                         &R.bhq, &R.bhq_pre, &R.bpop, &R.bpop_pre, &R.bex, &R.bex_pre})
        *p = c.take<uint32_t>(nb);
    if (plan)
        *plan = R;
    return c.at;
}

hipError_t launch_rfc_scans(hipStream_t s, const Batch& b, const wsg_stream_state* state, uint64_t msg_cap,
                            const MsgOut& o, const MsgScratch& x)
{
    const MsgPlan& P = x.plans.ref;
    const RfcPlan& R = x.plans.rfc;
    const uint32_t nb = uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK);
    k_rfc_scan_local<<<nb, BLOCK, 0, s>>>(b.wire, b.wire_len, b.fs, b.n, b.stream_first, b.n_streams, o.info, P.sidx, R,
                                          x.err);
    k_rfc_scan_blocks<<<1, BLOCK, 0, s>>>(R, nb);
    k_rfc_bytes_local<<<nb, BLOCK, 0, s>>>(o.info, b.n, state, P.sidx, R);
    k_rfc_bytes_blocks<<<1, BLOCK, 0, s>>>(P.tot, R, nb, b.n, msg_cap, o.count, x.err);
    return hipGetLastError();
}

hipError_t launch_rfc_finalize(hipStream_t s, const Batch& b, const MsgOut& o, const MsgScratch& x)
{
    k_rfc_finalize<<<uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK), BLOCK, 0, s>>>(
        b.wire, o.info, b.n, x.plans.ref.sidx, x.plans.rfc, o.msgs, x.pieces, x.pieces_cap);
    return hipGetLastError();
}

hipError_t launch_rfc_state(hipStream_t s, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                            wsg_stream_state* state, const RfcPlan& R, bool consumed_only)
{
    const uint32_t grid = uint32_t((uint64_t(n_streams) + BLOCK - 1) / BLOCK);
    const auto k = consumed_only ? k_rfc_state<true> : k_rfc_state<false>;
    k<<<grid, BLOCK, 0, s>>>(n, stream_first, n_streams, state, R);
    return hipGetLastError();
}

hipError_t launch_rfc_reply_local(hipStream_t s, bool checked, const Batch& b, const MsgOut& o, const MsgScratch& x,
                                  const ReplyRule& rule, const uint64_t* verdict)
{
    const uint32_t nb = uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK);
    const auto k = checked ? k_rfc_reply_local<true> : k_rfc_reply_local<false>;
    k<<<nb, BLOCK, 0, s>>>(b.wire, o.info, b.n, x.plans.ref, x.plans.rfc, rule, o.msgs, verdict);
    return hipGetLastError();
}

hipError_t launch_rfc_reply_finalize(hipStream_t s, bool checked, const Batch& b, const MsgOut& o, const MsgScratch& x,
                                     const ReplyOut& r, const ReplyRule& rule, const uint64_t* verdict)
{
    const uint32_t nb = uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK);
    const auto k = checked ? k_rfc_reply_finalize<true> : k_rfc_reply_finalize<false>;
    k<<<nb, BLOCK, 0, s>>>(o.info, b.n, b.stream_first, b.n_streams, x.plans.ref, x.plans.rfc, rule, r.send_key, o.msgs,
                           r.reply, r.reply_cap, r.reply_off, r.stream_reply, x.pieces, x.pieces_cap, verdict,
                           r.close_off);
    return hipGetLastError();
}

} // namespace wsg
