// wsg_proto.hip — the frame-sequence rules of RFC 6455 over a decoded batch
// (wsg_check_protocol).
#include "wsg_device.h"
#include "wsg_proto.h"

namespace wsg {

// ---- protocol rules on the device (wsg_check_protocol) ----------------------
// A frame's verdict needs its stream's state in front of it: whether a data
// message is open and how many bytes it holds (wsg_proto.h).  Every frame is a
// step on that state, "keep", "add len and set open" or "set (len, open)",
// and steps compose associatively, so the state before frame i is an exclusive
// scan of the steps over the frame table.  The segments are the streams: the
// step of a stream's first frame is taken behind the step that sets the
// stream's incoming state (d_proto[j]), which makes it a "set" and cuts it off
// from everything in front of it.  The structure is the message plan's:
//   k_proto_local   one lane per frame: the frame's stream (stored for the
//                   judge), its step, the block's composed step; a lane per
//                   stream seeds d_verdict (all 0xFF), the first lanes d_result
//   k_proto_blocks  one block over the block partials
//   k_proto_judge   one lane per frame: the block-local scan again, the state
//                   before the frame, its code; a frame with a code goes to
//                   d_verdict[j] by a 64-bit atomicMin of the verdict word
//                   (frame index on top: the first one wins), so valid traffic
//                   issues no atomic; the lane of the frame d_proto asks for
//                   leaves the state behind it in the plan
//   k_proto_finish  one lane per stream: d_proto (from the plan; d_proto is
//                   read by the two frame kernels, so none of them writes it),
//                   and d_result's counts, one atomic of each per wave that
//                   has something to add
//   k_proto_merge   wsg_reply_checked with d_also only, in front of the finish:
//                   one lane per stream, the other verdict where it comes first
// Work is proportional to frames plus streams; no lane walks a stream.

namespace {

// ProtoStep as block_scan_ex's element: 0 is the identity ("keep").
struct ProtoEl : ProtoStep {
    ProtoEl() = default;
    __device__ ProtoEl(int) : ProtoStep{0, PROTO_KEEP, 0} {}
    __device__ ProtoEl(const ProtoStep& s) : ProtoStep(s) {}
};
static_assert(sizeof(ProtoEl) == 16, "ProtoEl");

struct OpProto {
    __device__ __forceinline__ ProtoEl operator()(ProtoEl a, ProtoEl b) const { return proto_then(a, b); }
};

// (block_scan_ex forms inc - v for every element type and keeps it for a sum only)
__device__ __forceinline__ ProtoEl operator-(const ProtoEl& a, const ProtoEl&) { return a; }

// block_scan_ex's shuffle, for the element (found there by its argument's namespace)
__device__ __forceinline__ ProtoEl __shfl_up(const ProtoEl& v, unsigned int delta, int width)
{
    ProtoEl r;
    r.bytes = ::__shfl_up(v.bytes, delta, width);
    const uint32_t ko = ::__shfl_up(v.kind | (v.open << 2), delta, width);
    r.kind = ko & 3u;
    r.open = ko >> 2;
    return r;
}

__device__ __forceinline__ ProtoFrame load_frame(const wsg_recv_info* __restrict__ info, uint32_t i)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(info + i);
    return proto_frame(w[0], w[1], w[2], w[3]);
}

static_assert(sizeof(wsg_proto_state) == 16 && offsetof(wsg_proto_state, open) == 8, "wsg_proto_state layout");
static_assert(sizeof(wsg_proto_verdict) == 8 && offsetof(wsg_proto_verdict, status) == 2 &&
                  offsetof(wsg_proto_verdict, frame) == 4,
              "wsg_proto_verdict layout");

// d_proto[j] as the step that sets it.
__device__ __forceinline__ ProtoStep load_state(const wsg_proto_state* p)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    return proto_seed(w[0], (w[1] & 0xFFu) != 0);
}

__device__ __forceinline__ void store_state(uint64_t* w, const ProtoStep& s)
{
    w[0] = s.bytes;
    w[1] = s.open;   // _pad as 0
}

// One past the frame whose state d_proto[j] gets, for a stream [start, end):
// its end, or start + consumed.
__device__ __forceinline__ uint64_t proto_target(const wsg_stream_state* __restrict__ state, uint32_t j, uint32_t start,
                                                 uint32_t end)
{
    return state ? uint64_t(start) + state[j].consumed : uint64_t(end);
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_proto_local(const wsg_recv_info* __restrict__ info, uint32_t n,
                                                       const uint32_t* __restrict__ sf, uint32_t ns,
                                                       const wsg_proto_state* __restrict__ proto, ProtoPlan P,
                                                       uint32_t nb, unsigned long long* __restrict__ verdict,
                                                       uint64_t* __restrict__ result)
{
    // (a kernel's stores, not memsets: wsg_utf8.hip, k_utf8_init)
    if (blockIdx.x == 0 && threadIdx.x < 3)
        result[threadIdx.x] = threadIdx.x == 1 ? UINT64_MAX : 0;
    for (uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; j < ns; j += uint64_t(gridDim.x) * BLOCK)
        verdict[j] = ~0ull;
    if (blockIdx.x >= nb)
        return;   // a block that only seeds
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    ProtoEl el(0);
    if (i64 < n) {
        const uint32_t j = stream_of(sf, ns, i);
        P.sidx[i] = j;
        el = proto_step(load_frame(info, i));
        if (sf[j] == i)
            el = proto_then(load_state(proto + j), el);
    }
    ProtoEl tot;
    block_scan_ex(el, OpProto{}, &tot);
    if (threadIdx.x == 0)
        P.part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(BLOCK) void k_proto_blocks(ProtoPlan P, uint32_t nb)
{
    scan_partials(static_cast<const ProtoEl*>(P.part), static_cast<ProtoEl*>(P.pre), nb, OpProto{});
}

__global__ __launch_bounds__(BLOCK) void k_proto_judge(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                       const wsg_recv_info* __restrict__ info, uint32_t n,
                                                       const uint32_t* __restrict__ sf,
                                                       const wsg_stream_state* __restrict__ state,
                                                       const wsg_proto_state* __restrict__ proto, uint32_t role,
                                                       uint64_t max_message, ProtoPlan P,
                                                       unsigned long long* __restrict__ verdict)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    const uint32_t i = uint32_t(i64);
    ProtoFrame f{};
    ProtoStep step{0, PROTO_KEEP, 0}, seed{0, PROTO_KEEP, 0};
    uint32_t j = 0;
    bool head = false;
    if (i64 < n) {
        j = P.sidx[i];
        f = load_frame(info, i);
        step = proto_step(f);
        head = sf[j] == i;
        if (head)
            seed = load_state(proto + j);
    }
    ProtoEl tot;
    const ProtoEl ex = block_scan_ex(ProtoEl(proto_then(seed, step)), OpProto{}, &tot);
    if (i64 >= n)
        return;
    // (behind its stream's first frame the prefix is a "set": the whole state)
    const ProtoStep before = head ? seed : proto_then(static_cast<const ProtoEl*>(P.pre)[blockIdx.x], ex);
    const ProtoStep after = proto_then(before, step);
    uint32_t status;
    const uint32_t code = proto_code(
        f, before.open != 0, after.bytes, role, max_message,
        [&]() -> uint32_t {
            if (f.payload_off >= wire_len || wire_len - f.payload_off < 2)
                return 0u;
            return proto_wire_status(wire[f.payload_off], wire[f.payload_off + 1], f);
        },
        &status);
    if (code)
        atomicMin(verdict + j, static_cast<unsigned long long>(proto_verdict_word(code, status, i)));
    if (i64 + 1 == proto_target(state, j, sf[j], min(sf[j + 1], n)))
        store_state(P.out + 2 * uint64_t(j), after);
}

__global__ __launch_bounds__(BLOCK) void k_proto_finish(uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns,
                                                        const wsg_stream_state* __restrict__ state,
                                                        wsg_proto_state* proto, ProtoPlan P,
                                                        const uint64_t* __restrict__ verdict,
                                                        unsigned long long* __restrict__ result)
{
    uint64_t bad = 0, lowest = UINT64_MAX, closed = 0;
    for (uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; j64 < ns; j64 += uint64_t(gridDim.x) * BLOCK) {
        const uint32_t j = uint32_t(j64);
        const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
        const uint64_t target = proto_target(state, j, start, end);
        uint64_t* w = reinterpret_cast<uint64_t*>(proto + j);
        if (target > start && target <= end) {   // k_proto_judge left it
            w[0] = P.out[2 * j64];
            w[1] = P.out[2 * j64 + 1];
        } else {
            w[1] = (w[1] & 0xFFu) != 0;   // the incoming state, _pad as 0
        }
        const uint64_t v = verdict[j];
        const uint32_t code = uint32_t(v) & 0xFFu;
        if (v != UINT64_MAX && code >= WSG_PV_FRAME) {
            bad += 1;
            lowest = min(lowest, j64);
        }
        closed += v != UINT64_MAX && code == WSG_PV_CLOSED;
    }
    bad = wave_sum(bad);
    lowest = wave_min(lowest);
    closed = wave_sum(closed);
    if ((threadIdx.x & 63) != 0)
        return;
    if (bad) {
        atomicAdd(result, static_cast<unsigned long long>(bad));
        atomicMin(result + 1, static_cast<unsigned long long>(lowest));
    }
    if (closed)
        atomicAdd(result + 2, static_cast<unsigned long long>(closed));
}

// wsg_reply_checked's merge, one lane per stream between the judge and
// k_proto_finish (so that d_result counts what it leaves): d_verdict[j]
// becomes the caller's other verdict when that names a frame of the stream
// and comes first: a lower frame, or the same frame where the protocol's is a
// clean close and the other a violation.  All 0xFF in `also`: none.
__global__ __launch_bounds__(BLOCK) void k_proto_merge(uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns,
                                                       const uint64_t* __restrict__ also, uint64_t* verdict)
{
    for (uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; j < ns; j += uint64_t(gridDim.x) * BLOCK) {
        const uint64_t a = also[j];
        const uint32_t frame = uint32_t(a >> 32);
        const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
        if (a == UINT64_MAX || frame < start || frame >= end)
            continue;
        const uint64_t v = verdict[j];   // (all 0xFF: frame UINT32_MAX, behind every frame)
        const uint32_t vf = uint32_t(v >> 32);
        const uint32_t vcode = uint32_t(v) & 0xFFu, acode = uint32_t(a) & 0xFFu;
        if (frame < vf || (frame == vf && vcode == WSG_PV_CLOSED && acode >= WSG_PV_FRAME))
            verdict[j] = a;
    }
}

uint64_t proto_plan_layout(uint8_t* base, uint32_t n, uint32_t ns, ProtoPlan* plan)
{
    const uint64_t nb = (uint64_t(n) + BLOCK - 1) / BLOCK;
    Carve c{base, 16};
    ProtoPlan P;
    P.part = c.take<ProtoStep>(nb);
    P.pre = c.take<ProtoStep>(nb);
    P.out = c.take<uint64_t>(2 * uint64_t(ns));
    P.sidx = c.take<uint32_t>(n);
    if (plan)
        *plan = P;
    return c.at;
}

hipError_t launch_proto_scan(hipStream_t s, const Batch& b, const wsg_recv_info* info, const ProtoOps& p,
                             const ProtoPlan& plan)
{
    // with no stream no frame has one: nothing is judged
    const uint32_t nb = b.n_streams ? uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK) : 0u;
    const uint32_t seed_blocks = uint32_t((uint64_t(b.n_streams) + BLOCK - 1) / BLOCK);
    k_proto_local<<<max(max(nb, seed_blocks), 1u), BLOCK, 0, s>>>(info, b.n, b.stream_first, b.n_streams, p.proto, plan,
                                                                  nb, reinterpret_cast<unsigned long long*>(p.verdict),
                                                                  p.result);
    if (nb)
        k_proto_blocks<<<1, BLOCK, 0, s>>>(plan, nb);
    return hipGetLastError();
}

hipError_t launch_proto_judge(hipStream_t s, const Batch& b, const wsg_recv_info* info,
                              const wsg_stream_state* state, const ProtoOps& p, const ProtoPlan& plan)
{
    const uint32_t nb = uint32_t((uint64_t(b.n) + BLOCK - 1) / BLOCK);
    k_proto_judge<<<nb, BLOCK, 0, s>>>(b.wire, b.wire_len, info, b.n, b.stream_first, state, p.proto, p.role,
                                       p.max_message, plan, reinterpret_cast<unsigned long long*>(p.verdict));
    return hipGetLastError();
}

hipError_t launch_proto_merge(hipStream_t s, int grid, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                              const wsg_proto_verdict* also, wsg_proto_verdict* verdict)
{
    k_proto_merge<<<grid, BLOCK, 0, s>>>(n, stream_first, n_streams, reinterpret_cast<const uint64_t*>(also),
                                         reinterpret_cast<uint64_t*>(verdict));
    return hipGetLastError();
}

hipError_t launch_proto_finish(hipStream_t s, int grid, const Batch& b, const wsg_stream_state* state,
                               const ProtoOps& p, const ProtoPlan& plan)
{
    k_proto_finish<<<grid, BLOCK, 0, s>>>(b.n, b.stream_first, b.n_streams, state, p.proto, plan,
                                          reinterpret_cast<const uint64_t*>(p.verdict),
                                          reinterpret_cast<unsigned long long*>(p.result));
    return hipGetLastError();
}

} // namespace wsg
