// wsg_frames.hip — the device framer (wsg_frame_streams, wsg_decode_streams).
#include "wsg_device.h"

namespace wsg {

// ---- the device framer (wsg_frame_streams) ---------------------------------
// Frame boundaries are sequential within a connection and independent across
// connections: one wave walks one stream (grid-stride over streams).  Dense
// output needs every stream's count before a start can be written, so the
// streams are walked twice with a scan between: k_frame_count (consumed, need,
// count, span errors), k_frame_scan_local / k_frame_scan_blocks (exclusive
// prefix of the counts, d_count, the capacity latch), k_frame_write (the same
// walk again, its lines now in L2, storing the starts).
//
// The walk (frame_walk): the wave keeps a window of its stream in LDS, a ring
// of two halves of FR_HALF bytes, one aligned 16-B block per lane per half,
// lanes past the span's end loading nothing.  Plain loads: k_decode reads
// these lines next.  While half k is walked, half k + 1 is in the ring too (a
// header that starts in half k ends there at the latest) and half k + 2 is in
// flight in registers; it goes into half k's place once the position has left
// half k.  The position is wave-uniform: the header bytes parse_header asks
// for are read from the ring one by one (every lane the same LDS address, a
// broadcast read; one byte decides a short frame) and carried in scalar
// registers through uni().  A frame that ends beyond
// the ring is a jump: the ring is re-based at the new position (one memory
// round trip) and the payload between is never loaded.  The 64 most recent
// starts wait in the lanes (lane i the i-th) and leave in one 512-byte store.
//
// Limits: one stream's walk is serial (an LDS round trip and some sixty
// mostly scalar instructions per frame), so a batch that is one connection of tiny
// frames is latency-bound on one wave, and one long stream among short ones
// is the launch's critical path.

namespace {

constexpr uint32_t FR_HALF = 64 * CHUNK;          // 1 KiB: a 16-B block per lane
constexpr uint32_t FR_BLOCKS = 2 * FR_HALF / 16;  // 16-B blocks of a wave's ring
static_assert((FR_BLOCKS & (FR_BLOCKS - 1)) == 0 && FR_HALF >= 32, "the ring index is a mask; a header spans two blocks");

// The aligned 16-B block at wire offset a, nothing for a block past `end`
// (end <= wire_len, and the wire is readable to the end of its last block).
__device__ __forceinline__ v4u fr_load(const uint8_t* __restrict__ wire, uint64_t a, uint64_t end)
{
    return a < end ? ld16(wire + a) : v4u{0, 0, 0, 0};
}

// Walk the whole frames of wire[off, end).  WRITE: store at most max_frames
// starts to out[0..).  Every argument is wave-uniform.
template <bool WRITE>
__device__ __forceinline__ void frame_walk(const uint8_t* __restrict__ wire, uint64_t off, uint64_t end, v4u* ring,
                                           uint64_t* __restrict__ out, uint64_t max_frames, uint64_t& consumed,
                                           uint64_t& need, uint64_t& count)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t pos = off, cnt = 0, mine = 0;
    uint64_t base = 0;   // wire offset of ring block 0 (16-B aligned)
    uint64_t hs = 0;     // start of the half being walked; [hs, hs + 2 * FR_HALF) is in the ring
    v4u pre = v4u{0, 0, 0, 0};   // the half behind those, in flight
    bool fresh = true;
    need = 0;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(ring);
    bool done = false;
    while (!done) {
        if (pos == end)   // need = 0
            break;
        if (fresh || pos - hs >= 2 * uint64_t(FR_HALF)) {   // a jump: re-base the ring at pos
            fresh = false;
            base = hs = pos & ~uint64_t(15);
            const uint64_t a = base + uint64_t(lane) * CHUNK;
            const v4u v0 = fr_load(wire, a, end), v1 = fr_load(wire, a + FR_HALF, end);
            pre = fr_load(wire, a + 2 * uint64_t(FR_HALF), end);
            ring[lane] = v0;
            ring[64 + lane] = v1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else if (pos - hs >= FR_HALF) {   // left a half: the one in flight takes its place
            ring[(uint32_t((hs - base) >> 4) + lane) & (FR_BLOCKS - 1)] = pre;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            hs += FR_HALF;
            pre = fr_load(wire, hs + 2 * uint64_t(FR_HALF) + uint64_t(lane) * CHUNK, end);
        }
        // the frames that start in this half: nothing but LDS reads and
        // scalar arithmetic (and, WRITE, a store every 64 frames) in here
        const uint64_t lim = min(hs + FR_HALF, end);
        while (pos < lim) {
            const uint64_t rem = end - pos;
            if (rem < 2) {
                need = 2;
                done = true;
                break;
            }
            if (WRITE && cnt >= max_frames) {
                done = true;
                break;
            }
            // header bytes as parse_header asks for them: broadcast LDS reads
            // of the ring ([hs, hs + 2 * FR_HALF) holds any header that starts
            // before lim), each made a scalar
            const uint32_t at = uint32_t(pos - base);
            const auto byte_at = [&](uint32_t k) { return uint8_t(uni(uint32_t(bytes[(at + k) & (16 * FR_BLOCKS - 1)]))); };
            wsg_recv_info r;
            if (parse_header(byte_at, rem, r) != 0) {   // rem >= 2: the header is incomplete
                need = header_len(byte_at(1));
                done = true;
                break;
            }
            const uint32_t hdr = r.hdr_len;
            if (r.len > rem - hdr) {   // (no hdr + len: a 127-form length may be 2^64 - 1)
                need = r.len > UINT64_MAX - hdr ? UINT64_MAX : hdr + r.len;
                done = true;
                break;
            }
            if (WRITE) {
                if (lane == uint32_t(cnt & 63))
                    mine = pos;
                if ((cnt & 63) == 63)
                    out[cnt - 63 + lane] = mine;
            }
            ++cnt;
            pos += hdr + r.len;
        }
    }
    if (WRITE && lane < uint32_t(cnt & 63))
        out[(cnt & ~uint64_t(63)) + lane] = mine;
    consumed = pos - off;
    count = cnt;
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_frame_count(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                       wsg_stream_span* span, uint32_t ns, uint64_t* __restrict__ cnt,
                                                       unsigned long long* err)
{
    __shared__ v4u s_ring[BLOCK / 64][FR_BLOCKS];
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63, wid = wave_id();
    for (uint64_t j64 = uint64_t(blockIdx.x) * (BLOCK / 64) + wid; j64 < ns; j64 += waves) {
        const uint32_t j = uint32_t(j64);
        const SpanIn s = span_in(span, j, wire_len);
        uint64_t consumed = 0, need = 0, n = 0;
        if (s.ok)
            frame_walk<false>(wire, s.off, s.off + s.len, s_ring[wid], nullptr, 0, consumed, need, n);
        if (lane == 0) {
            if (!s.ok)
                latch(err, j, WSG_EINVAL);
            uint64_t* w = reinterpret_cast<uint64_t*>(span + j);
            w[2] = consumed;
            w[3] = need;
            cnt[j] = n;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_frame_scan_local(const wsg_stream_span* span, uint32_t ns, FramePlan P)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    uint64_t c = 0, k = 0;
    if (j64 < ns) {
        c = P.cnt[j64];
        k = reinterpret_cast<const uint64_t*>(span + j64)[2];
    }
    uint64_t tc, tk;
    const uint64_t ec = block_scan_ex(c, OpAdd{}, &tc);
    (void)block_scan_ex(k, OpAdd{}, &tk);
    if (j64 < ns)
        P.ex[j64] = ec;
    if (threadIdx.x == 0) {
        P.bcnt[blockIdx.x] = tc;
        P.bcons[blockIdx.x] = tk;
    }
}

__global__ __launch_bounds__(BLOCK) void k_frame_scan_blocks(FramePlan P, uint32_t nb, uint32_t ns, uint32_t frame_cap,
                                                             uint64_t* __restrict__ count, unsigned long long* err)
{
    const uint64_t cc = scan_partials(P.bcnt, P.bpre, nb, OpAdd{});
    const uint64_t ck = scan_partials<uint64_t>(P.bcons, nullptr, nb, OpAdd{});
    if (threadIdx.x == 0) {
        P.tot[0] = cc;
        P.tot[1] = ck;
        count[0] = cc;
        count[1] = ck;
        // behind every span error: the latch keeps the smallest
        if (cc > uint64_t(UINT32_MAX) - 1)
            latch(err, ns, WSG_EINVAL);
        else if (cc > frame_cap)
            latch(err, ns, WSG_ENOMEM);
    }
}

__global__ __launch_bounds__(BLOCK) void k_frame_write(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                       const wsg_stream_span* span, uint32_t ns, FramePlan P,
                                                       uint64_t* __restrict__ fs, uint32_t frame_cap,
                                                       uint32_t* __restrict__ sf)
{
    __shared__ v4u s_ring[BLOCK / 64][FR_BLOCKS];
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63, wid = wave_id();
    const uint64_t total = uni(P.tot[0]);
    // WSG_ENOMEM / WSG_EINVAL latched by k_frame_scan_blocks: no entry of fs
    const bool fits = total <= frame_cap && total <= uint64_t(UINT32_MAX) - 1;
    for (uint64_t j64 = uint64_t(blockIdx.x) * (BLOCK / 64) + wid; j64 < ns; j64 += waves) {
        const uint32_t j = uint32_t(j64);
        const uint64_t first = uni(P.ex[j] + P.bpre[j / BLOCK]);
        const uint64_t next = j64 + 1 < ns ? uni(P.ex[j + 1] + P.bpre[(j + 1) / BLOCK]) : total;
        if (lane == 0) {
            sf[j] = uint32_t(min(first, uint64_t(UINT32_MAX)));
            if (j64 + 1 == ns)
                sf[ns] = uint32_t(min(total, uint64_t(UINT32_MAX)));
        }
        if (!fits || next <= first)
            continue;
        const SpanIn s = span_in(span, j, wire_len);
        if (!s.ok)
            continue;
        uint64_t consumed, need, n;
        frame_walk<true>(wire, s.off, s.off + s.len, s_ring[wid], fs + first, next - first, consumed, need, n);
    }
}

// One lane per stream.
__global__ __launch_bounds__(BLOCK) void k_frame_tail(wsg_stream_span* span, uint32_t ns,
                                                      const uint64_t* __restrict__ fs,
                                                      const uint32_t* __restrict__ sf,
                                                      const wsg_stream_state* __restrict__ state, uint32_t n)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    const uint32_t start = min(sf[j64], n), end = max(min(sf[j64 + 1], n), start);
    const uint32_t used = state[j64].consumed;
    if (used < end - start) {
        uint64_t* w = reinterpret_cast<uint64_t*>(span + j64);
        w[2] = fs[start + used] - w[0];
    }
}

uint64_t frame_plan_layout(uint64_t* base, uint32_t ns, FramePlan* plan)
{
    const uint64_t nb = (uint64_t(ns) + BLOCK - 1) / BLOCK;
    Carve c{reinterpret_cast<uint8_t*>(base), sizeof(uint64_t)};
    FramePlan P;
    P.cnt = c.take<uint64_t>(ns);
    P.ex = c.take<uint64_t>(ns);
    P.bcnt = c.take<uint64_t>(nb);
    P.bpre = c.take<uint64_t>(nb);
    P.bcons = c.take<uint64_t>(nb);
    P.tot = c.take<uint64_t>(2);
    if (plan)
        *plan = P;
    return c.at / sizeof(uint64_t);
}

hipError_t launch_frame_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len, wsg_stream_span* span,
                                uint32_t ns, uint64_t* frame_start, uint32_t frame_cap, uint32_t* stream_first,
                                uint64_t* count, const FramePlan& plan, unsigned long long* err)
{
    if (ns == 0) {   // no stream: no frame
        if (hipError_t e = hipMemsetAsync(count, 0, 2 * sizeof(uint64_t), s); e != hipSuccess)
            return e;
        return hipMemsetAsync(stream_first, 0, sizeof(uint32_t), s);
    }
    const uint32_t nb = uint32_t((uint64_t(ns) + BLOCK - 1) / BLOCK);
    k_frame_count<<<grid, BLOCK, 0, s>>>(wire, wire_len, span, ns, plan.cnt, err);
    k_frame_scan_local<<<nb, BLOCK, 0, s>>>(span, ns, plan);
    k_frame_scan_blocks<<<1, BLOCK, 0, s>>>(plan, nb, ns, frame_cap, count, err);
    k_frame_write<<<grid, BLOCK, 0, s>>>(wire, wire_len, span, ns, plan, frame_start, frame_cap, stream_first);
    return hipGetLastError();
}

hipError_t launch_frame_tail(hipStream_t s, wsg_stream_span* span, uint32_t ns, const uint64_t* frame_start,
                             const uint32_t* stream_first, const wsg_stream_state* state, uint32_t n)
{
    if (ns == 0 || n == 0)
        return hipSuccess;
    k_frame_tail<<<(ns + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(span, ns, frame_start, stream_first, state, n);
    return hipGetLastError();
}

} // namespace wsg
