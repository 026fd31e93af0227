// wsg_carry.hip — the carry between two rounds (wsg_carry_streams).
#include "wsg_device.h"

namespace wsg {

// ---- the carry (wsg_carry_streams) -------------------------------------------
// The next round's wire is, per stream, what the last round left unconsumed
// (the tail, wire[off + consumed, off + len)) followed by what the host has
// just read (new[read.off, read.off + read.len)).  Like the framer's, its
// shape is per-stream sizes, a scan, and a ragged copy:
//   k_carry_sizes        one lane per stream: tail and read as source runs, the
//                        per-stream errors; block-local scan of the padded sizes
//   k_carry_scan_blocks  those over the block partials; d_count; WSG_ENOMEM
//   k_carry_spans        one lane per stream: its offset in d_next, d_next_span
//   k_carry_copy         every 16-byte chunk of d_next[0, d_count[0]) once
// A stream starts on a 16-byte chunk of d_next, so a chunk belongs to one
// stream and holds bytes of at most two source runs and the padding, and
// every store is one whole aligned 16-byte store.
//
// The copy (k_carry_copy) takes d_next in pieces of PIECE bytes, a wave each,
// grid-stride.  A piece inside ONE run of ONE stream is k_msg_gather's copy:
// the source shift is uniform over the wave, one aligned nontemporal load per
// lane and chunk, the second block of the 32-byte window from the next lane's
// registers, a funnel, a nontemporal store.  Any other piece (a run's end, a
// stream's end, many small streams) finds each chunk's stream per lane, by a
// search between the streams of the piece's first and last chunk, and builds
// the chunk from the windows of the two runs, each at most two aligned blocks, masked to the run's bytes and ORed: the chunk that
// straddles tail and read comes out of registers, the padding is the zeros
// left where neither run has a byte.  Plain loads there: neighbouring lanes
// read the same blocks.  The streams of a piece's first and last chunk are
// found by the whole wave (stream_of64_wave: two or three dependent loads
// where a binary search has twelve to sixteen in front of the piece's first
// data load; tools/carrybench.py, profiles/r19: 29.7 -> 25.6 us on 65536
// small streams, 95.3 -> 93.9 us on 4096 of 64 KiB).

namespace {

// 16 bytes of a run as seen from a chunk: byte k = run[c + k] where c + k lies
// inside [0, len), else 0.  Reads only aligned 16-byte blocks that hold a
// wanted byte, at most two.
__device__ __forceinline__ v4u run_window(const uint8_t* __restrict__ run, uint64_t len, int64_t c)
{
    const int64_t n = int64_t(len);
    if (c >= n || c + CHUNK <= 0)
        return v4u{0, 0, 0, 0};
    const uint32_t s = uint32_t((reinterpret_cast<uintptr_t>(run) + uint64_t(c)) & 15u);
    const int64_t r0 = c - int64_t(s);   // the aligned block holding byte c, relative to run
    v4u lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (r0 + CHUNK > 0)
        lo = ld16(run + r0);
    if (s != 0 && r0 + CHUNK < n)
        hi = ld16(run + r0 + CHUNK);
    v4u v = s ? funnel(lo, hi, s) : lo;
    v &= low_bytes(uint64_t(n - c));
    if (c < 0)
        v &= ~low_bytes(uint64_t(-c));
    return v;
}

} // namespace

// One lane per stream.
__global__ __launch_bounds__(BLOCK) void k_carry_sizes(uint64_t wire_len, const wsg_stream_span* __restrict__ span,
                                                       uint32_t ns, const uint64_t* __restrict__ close_off,
                                                       uint64_t new_len, const wsg_stream_read* __restrict__ read,
                                                       CarryPlan P, unsigned long long* err)
{
    static_assert(sizeof(wsg_stream_read) == 16, "wsg_stream_read layout");
    const uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    uint64_t tsrc = 0, tlen = 0, nsrc = 0, nlen = 0, drop = 0;
    if (j < ns) {
        const SpanLane s = span_in_lane(span, j, wire_len);
        bool bad = !s.ok || s.consumed > s.len;
        drop = close_off && close_off[j] != UINT64_MAX;
        if (!bad && !drop) {   // (a dropped stream's read is ignored, whatever it holds)
            tsrc = s.off + s.consumed;
            tlen = s.len - s.consumed;
            if (read) {
                const uint64_t* r = reinterpret_cast<const uint64_t*>(read + j);
                nsrc = r[0];
                nlen = r[1];
                if (nsrc > new_len || nlen > new_len - nsrc)
                    bad = true;
            }
        }
        if (bad) {
            latch(err, j, WSG_EINVAL);
            tlen = nlen = 0;
        }
        P.tsrc[j] = tsrc;
        P.tlen[j] = tlen;
        P.nsrc[j] = nsrc;
        P.nlen[j] = nlen;
    }
    const uint64_t size = (tlen + nlen + (CHUNK - 1)) & ~uint64_t(CHUNK - 1);
    uint64_t ts, tt, tn, td;
    const uint64_t ex = block_scan_ex(size, OpAdd{}, &ts);
    (void)block_scan_ex(tlen, OpAdd{}, &tt);
    (void)block_scan_ex(nlen, OpAdd{}, &tn);
    (void)block_scan_ex(drop, OpAdd{}, &td);
    if (j < ns)
        P.ex[j] = ex;
    if (threadIdx.x == 0) {
        const uint64_t nb = gridDim.x;
        P.bsum[blockIdx.x] = ts;
        P.bsum[nb + blockIdx.x] = tt;
        P.bsum[2 * nb + blockIdx.x] = tn;
        P.bsum[3 * nb + blockIdx.x] = td;
    }
}

__global__ __launch_bounds__(BLOCK) void k_carry_scan_blocks(CarryPlan P, uint32_t nb, uint32_t ns, uint64_t next_cap,
                                                             uint64_t* __restrict__ count, unsigned long long* err)
{
    const uint64_t ts = scan_partials(P.bsum, P.bpre, nb, OpAdd{});
    const uint64_t tt = scan_partials<uint64_t>(P.bsum + nb, nullptr, nb, OpAdd{});
    const uint64_t tn = scan_partials<uint64_t>(P.bsum + 2 * uint64_t(nb), nullptr, nb, OpAdd{});
    const uint64_t td = scan_partials<uint64_t>(P.bsum + 3 * uint64_t(nb), nullptr, nb, OpAdd{});
    if (threadIdx.x == 0) {
        P.off[ns] = ts;
        count[0] = ts;
        count[1] = tt;
        count[2] = tn;
        count[3] = td;
        if (ts > next_cap)   // behind every stream's error: the latch keeps the smallest
            latch(err, ns, WSG_ENOMEM);
    }
}

// One lane per stream.
__global__ __launch_bounds__(BLOCK) void k_carry_spans(uint32_t ns, CarryPlan P, wsg_stream_span* __restrict__ next_span)
{
    const uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j >= ns)
        return;
    const uint64_t off = P.ex[j] + P.bpre[j / BLOCK];
    P.off[j] = off;
    uint64_t* w = reinterpret_cast<uint64_t*>(next_span + j);
    w[0] = off;
    w[1] = P.tlen[j] + P.nlen[j];
    w[2] = 0;
    w[3] = 0;
}

__global__ __launch_bounds__(BLOCK) void k_carry_copy(const uint8_t* __restrict__ wire, const uint8_t* __restrict__ fresh,
                                                      uint32_t ns, CarryPlan P, uint8_t* __restrict__ next,
                                                      uint64_t next_cap)
{
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t q0 = uint64_t(blockIdx.x) * (BLOCK / 64) + wave_id();
    const uint64_t total = uni(P.off[ns]);
    if (total > next_cap)
        return;   // WSG_ENOMEM latched by k_carry_scan_blocks: no byte of next
    const uint64_t pieces = (total + PIECE - 1) / PIECE;
    for (uint64_t q = q0; q < pieces; q += waves) {
        const uint64_t p0 = q * PIECE, p1 = min(p0 + PIECE, total);   // (total is a multiple of CHUNK)
        // the stream of the piece's first chunk (wave-uniform)
        const uint32_t j0 = stream_of64_wave(P.off, 0, ns, p0, lane);
        const uint64_t o = uni(P.off[j0]), tl = uni(P.tlen[j0]), nl = uni(P.nlen[j0]);
        const bool in_tail = p0 >= o && p1 <= o + tl, in_read = p0 >= o + tl && p1 <= o + tl + nl;
        if (in_tail || in_read) {
            // the source of byte p0; every chunk below p1 is 16 bytes of the run: k_msg_gather's copy
            const uint8_t* src = in_tail ? wire + uni(P.tsrc[j0]) + (p0 - o) : fresh + uni(P.nsrc[j0]) + (p0 - o - tl);
            const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(src) & 15u);
            v4u a[EU], b[EU];
            uint32_t full = 0;
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const uint64_t d = (uint64_t(u) * 64 + lane) * CHUNK;
                const bool f = p0 + d < p1;
                full |= uint32_t(f) << u;
                a[u] = f ? ld16nt(src + (int64_t(d) - int64_t(s))) : v4u{0, 0, 0, 0};
            }
            // bit u: the lane after this one in the piece (lane 0 of the next row
            // for lane 63) loaded the block after a[u] as its own first block
            const uint32_t nfull = lane == 63 ? uint32_t(__builtin_amdgcn_readlane(full, 0)) >> 1
                                              : uint32_t(__shfl_down(full, 1, 64));
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const uint64_t d = (uint64_t(u) * 64 + lane) * CHUNK;
                b[u] = ((full >> u) & 1u) && s && !((nfull >> u) & 1u) ? ld16nt(src + (int64_t(d) - int64_t(s)) + CHUNK)
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
#pragma unroll
            for (int u = 0; u < EU; ++u)
                a[u] = s ? funnel(a[u], b[u], s) : a[u];
#pragma unroll
            for (int u = 0; u < EU; ++u)
                if ((full >> u) & 1u)
                    st16nt(next + p0 + (uint64_t(u) * 64 + lane) * CHUNK, a[u]);
            continue;
        }
        // the stream of the piece's last chunk (wave-uniform), then each chunk's own
        const uint32_t j1 = stream_of64_wave(P.off, j0, ns, p1 - CHUNK, lane);
        v4u v[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = p0 + (uint64_t(u) * 64 + lane) * CHUNK;
            v[u] = v4u{0, 0, 0, 0};
            if (p < p1) {
                const uint32_t j = stream_of64(P.off, j0, j1 + 1, p);
                const int64_t r = int64_t(p - P.off[j]);   // the chunk's first byte in the stream
                const uint64_t t = P.tlen[j];
                v[u] = run_window(wire + P.tsrc[j], t, r) | run_window(fresh + P.nsrc[j], P.nlen[j], r - int64_t(t));
            }
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = p0 + (uint64_t(u) * 64 + lane) * CHUNK;
            if (p < p1)
                st16nt(next + p, v[u]);
        }
    }
}

uint64_t carry_plan_layout(uint64_t* base, uint32_t ns, CarryPlan* plan)
{
    const uint64_t nb = (uint64_t(ns) + BLOCK - 1) / BLOCK;
    Carve c{reinterpret_cast<uint8_t*>(base), sizeof(uint64_t)};
    CarryPlan P;
    P.tsrc = c.take<uint64_t>(ns);
    P.tlen = c.take<uint64_t>(ns);
    P.nsrc = c.take<uint64_t>(ns);
    P.nlen = c.take<uint64_t>(ns);
    P.ex = c.take<uint64_t>(ns);
    P.off = c.take<uint64_t>(uint64_t(ns) + 1);
    P.bsum = c.take<uint64_t>(4 * nb);
    P.bpre = c.take<uint64_t>(nb);
    if (plan)
        *plan = P;
    return c.at / sizeof(uint64_t);
}

hipError_t launch_carry_plan(hipStream_t s, uint64_t wire_len, const wsg_stream_span* span, uint32_t ns,
                             const uint64_t* close_off, uint64_t new_len, const wsg_stream_read* read, uint64_t next_cap,
                             wsg_stream_span* next_span, uint64_t* count, const CarryPlan& plan, unsigned long long* err)
{
    if (ns == 0)   // no stream: no byte
        return hipMemsetAsync(count, 0, 4 * sizeof(uint64_t), s);
    const uint32_t nb = uint32_t((uint64_t(ns) + BLOCK - 1) / BLOCK);
    k_carry_sizes<<<nb, BLOCK, 0, s>>>(wire_len, span, ns, close_off, new_len, read, plan, err);
    k_carry_scan_blocks<<<1, BLOCK, 0, s>>>(plan, nb, ns, next_cap, count, err);
    k_carry_spans<<<nb, BLOCK, 0, s>>>(ns, plan, next_span);
    return hipGetLastError();
}

hipError_t launch_carry_copy(hipStream_t s, int grid, const uint8_t* wire, const uint8_t* fresh, uint32_t ns,
                             const CarryPlan& plan, uint8_t* next, uint64_t next_cap)
{
    k_carry_copy<<<grid, BLOCK, 0, s>>>(wire, fresh, ns, plan, next, next_cap);
    return hipGetLastError();
}

} // namespace wsg
