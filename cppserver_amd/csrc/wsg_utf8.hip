// wsg_utf8.hip — UTF-8 validation of decoded messages (wsg_check_utf8).
#include "wsg_device.h"
#include "wsg_utf8.h"

namespace wsg {

// ---- UTF-8 on the device (wsg_check_utf8) ----------------------------------
// d_msg holds every message unmasked, its fragments joined: a text message
// (or a close reason) is one byte string there, and whether a position of it
// is bad depends on the 3 bytes before it and the 3 after (wsg_utf8.h).  So
// the payload kernel is element-wise over the aligned 16-byte chunks of
// d_msg[0, min(msg_cap, d_count[1])): one chunk per lane, one 16-B load, the
// 4 bytes on either side from the neighbouring lanes' registers (the wave's
// first and last lane load theirs).  A lane whose chunk holds no byte >= 0x80
// has no bad position and does nothing more; a wave of such lanes goes on to
// its next pass.  Otherwise the wave finds, with two searches of d_msgs
// (message ends are non-decreasing; 64 probes a round, one per lane), the
// records [mlo, mhi] its 1 KiB can touch, and each lane with a byte >= 0x80 walks the messages that overlap
// its chunk: the next record whose end lies beyond the position reached (a
// search inside [mlo, mhi], none when the wave lies in one message), so a run
// of empty messages at one offset costs one step, and a chunk at most 16.
// The bytes of the window outside the message in hand count as 00; the rule
// of wsg_utf8.h is asked about the chunk word-wise (utf8_words_bad, some 80
// VALU operations per 4 bytes), and only a lane it flags asks the
// position-local form about its 16 positions; the lowest bad one goes to
// d_valid[m] by atomicMin.  Valid text issues no
// atomic.  k_utf8_init (d_valid[m] = len, d_result's seed) runs before it and
// k_utf8_count (the four words of d_result) behind it, one lane per record.

namespace {

struct Utf8Rec {
    uint64_t off, len, end;   // end: off + len, saturating
    bool selected;
};

__device__ __forceinline__ Utf8Rec utf8_rec(const wsg_msg* __restrict__ msgs, uint32_t m, uint32_t which)
{
    const MsgRec g = get_msg(msgs + m);
    Utf8Rec r;
    r.off = g.off;
    r.len = g.len;
    r.end = msg_end(g.off, g.len);
    r.selected = (which & WSG_UTF8_EVERY) || ((which & WSG_UTF8_TEXT) && g.kind == WSG_CB_RECEIVED && g.op == WSG_TEXT) ||
                 ((which & WSG_UTF8_CLOSE) && g.kind == WSG_CB_CLOSE);
    return r;
}

// off + len <= bound, without forming the sum
__device__ __forceinline__ bool utf8_inside(const Utf8Rec& r, uint64_t bound)
{
    return r.len <= bound && r.off <= bound - r.len;
}

// First m in [lo, hi) whose end lies beyond pos; hi when there is none.
__device__ __forceinline__ uint32_t utf8_first_beyond(const wsg_msg* __restrict__ msgs, uint32_t lo, uint32_t hi,
                                                      uint64_t pos)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (msg_end(msgs, mid) > pos)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The same answer for a wave-uniform pos, found by the whole wave: 64 probes a
// round, the range shrinking 64-fold (two or three dependent loads where the
// one-lane search takes log2 M of them; a wave's two searches per pass were
// most of the time of non-ASCII text with the one-lane form).
__device__ __forceinline__ uint32_t utf8_first_beyond_wave(const wsg_msg* __restrict__ msgs, uint32_t lo, uint32_t hi,
                                                           uint64_t pos)
{
    const uint32_t lane = threadIdx.x & 63;
    while (lo < hi) {   // the answer lies in [lo, hi]
        const uint32_t step = (hi - lo + 63) / 64;
        const uint64_t idx = uint64_t(lo) + uint64_t(lane) * step;
        bool beyond = true;   // (a probe at or past hi counts as beyond)
        if (idx < hi)
            beyond = msg_end(msgs, idx) > pos;
        const uint64_t b = __ballot(beyond);
        const uint32_t f = b ? uint32_t(__builtin_ctzll(b)) : 64u;   // the first probe beyond pos
        if (f == 0) {
            hi = lo;
        } else {   // behind probe f - 1, at or before probe f
            const uint64_t top = uint64_t(lo) + uint64_t(f) * step;
            lo = lo + (f - 1) * step + 1;
            hi = top < hi ? uint32_t(top) : hi;
        }
    }
    return lo;
}

// n < 16 bytes at p, one by one (the chunk the bound cuts: no byte at or past it is read)
__device__ __forceinline__ v4u utf8_ld_partial(const uint8_t* __restrict__ p, uint32_t n)
{
    v4u r{0, 0, 0, 0};
    for (uint32_t t = 0; t < n; ++t)
        put_byte(r, t, p[t]);
    return r;
}

// Bit i: chunk position i lies in [lo, hi) and is bad in the string whose
// bytes are the window's bytes at the chunk-relative positions [lo, hi).  The
// window: pre = positions -4..-1, c = 0..15, post = 16..19.
__device__ __forceinline__ uint32_t utf8_chunk_bad(uint32_t pre, v4u c, uint32_t post, int lo, int hi)
{
    uint32_t d[6] = {pre, c.x, c.y, c.z, c.w, post};
    // dword k holds the positions 4k - 4 .. 4k - 1: 00 outside [lo, hi)
#pragma unroll
    for (int k = 0; k < 6; ++k)
        d[k] &= low_bytes(hi + 4 - 4 * k) & ~low_bytes(lo + 4 - 4 * k);
    // word-wise first (wsg_utf8.h): valid text, the common case, ends here
    uint32_t flags[4];
    utf8_words_bad(d, flags);
    if ((flags[0] | flags[1] | flags[2] | flags[3]) == 0)
        return 0;
    uint32_t by[22];   // positions -3..18 (constant indices once unrolled: registers)
#pragma unroll
    for (int j = 0; j < 22; ++j)
        by[j] = (d[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu;
    // (a position outside [lo, hi) now holds 00, an ASCII byte, never bad)
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        auto at = [&](int64_t k) { return by[k + 3]; };
        if (by[i + 3] >= 0x80u && utf8_bad_at(at, int64_t(i)))
            bad |= 1u << i;
    }
    return bad;
}

} // namespace

// One lane per record (grid-stride): d_valid[m] = len; the first lane seeds
// d_result = {0, UINT64_MAX, 0, 0} for k_utf8_count behind it.  (A kernel's
// stores, not memsets: the call is meant to be captured, and the two memset
// nodes this began with came back from a graph replay with other fill values.)
__global__ __launch_bounds__(BLOCK) void k_utf8_init(const wsg_msg* __restrict__ msgs,
                                                     const uint64_t* __restrict__ count, uint32_t msg_room,
                                                     uint64_t* __restrict__ valid, uint64_t* __restrict__ result)
{
    if (blockIdx.x == 0 && threadIdx.x < 4)
        result[threadIdx.x] = threadIdx.x == 1 ? UINT64_MAX : 0;
    const uint64_t M = min(count[0], uint64_t(msg_room));
    for (uint64_t m = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; m < M; m += uint64_t(gridDim.x) * BLOCK)
        valid[m] = msgs[m].len;
}

__global__ __launch_bounds__(BLOCK) void k_utf8_scan(const uint8_t* __restrict__ msg, uint64_t msg_cap,
                                                     const wsg_msg* __restrict__ msgs,
                                                     const uint64_t* __restrict__ count, uint32_t msg_room,
                                                     uint32_t which, unsigned long long* __restrict__ valid)
{
    const uint32_t M = uint32_t(min(count[0], uint64_t(msg_room)));
    const uint64_t bound = min(msg_cap, count[1]);
    if (M == 0)
        return;
    const uint32_t lane = threadIdx.x & 63;
    constexpr uint64_t WAVE_BYTES = 64 * CHUNK;
    const uint64_t stride = uint64_t(gridDim.x) * BLOCK * CHUNK;
    // (wave-uniform loop: every lane of a wave takes part in the shuffles)
    for (uint64_t wb = (uint64_t(blockIdx.x) * (BLOCK / 64) + wave_id()) * WAVE_BYTES; wb < bound; wb += stride) {
        const uint64_t p = wb + uint64_t(lane) * CHUNK;
        v4u c{0, 0, 0, 0};
        if (p < bound)
            c = bound - p >= CHUNK ? ld16nt(msg + p) : utf8_ld_partial(msg + p, uint32_t(bound - p));
        const bool hot = ((c.x | c.y | c.z | c.w) & 0x80808080u) != 0;   // a bad position is never an ASCII byte
        if (__ballot(hot) == 0)
            continue;
        uint32_t pre = uint32_t(__shfl_up(c.w, 1, 64)), post = uint32_t(__shfl_down(c.x, 1, 64));
        if (lane == 0)
            pre = wb ? *reinterpret_cast<const uint32_t*>(msg + wb - 4) : 0u;
        if (lane == 63) {
            const uint64_t q = p + CHUNK;
            post = 0;
            if (q < bound)
                post = bound - q >= 4 ? *reinterpret_cast<const uint32_t*>(msg + q)
                                      : utf8_ld_partial(msg + q, uint32_t(bound - q)).x;
        }
        // the records the wave's bytes [wb, wb + WAVE_BYTES) can lie in
        const uint32_t mlo = uni(utf8_first_beyond_wave(msgs, 0, M, wb));
        if (mlo >= M)
            return;   // no message ends beyond wb: nor beyond any later pass
        const uint32_t mhi = uni(utf8_first_beyond_wave(msgs, mlo, M, wb + (WAVE_BYTES - 1)));
        if (!hot)
            continue;
        uint64_t pos = p;
        uint32_t m = mlo;
#pragma unroll 1
        while (pos - p < CHUNK) {
            m = utf8_first_beyond(msgs, m, mhi, pos);
            if (m >= M)
                break;
            const Utf8Rec r = utf8_rec(msgs, m, which);
            if (r.end <= pos || r.off >= p + CHUNK)
                break;   // (the first: a table whose ends are not sorted)
            if (r.selected && utf8_inside(r, bound)) {
                const int lo = r.off >= p ? int(r.off - p) : p - r.off >= 4 ? -4 : -int(p - r.off);
                const int hi = r.end - p >= 20 ? 20 : int(r.end - p);
                const uint32_t bad = utf8_chunk_bad(pre, c, post, lo, hi);
                if (bad)
                    atomicMin(valid + m, static_cast<unsigned long long>(p + uint32_t(__builtin_ctz(bad)) - r.off));
            }
            pos = r.end;
        }
    }
}

// One lane per record (grid-stride), behind the scan: the checked messages
// with d_valid[m] < len (an unchecked one holds len), the lowest such m, the
// messages checked and their bytes into result[0..4) (seeded by k_utf8_init),
// one atomic of each per wave that has something to add.
__global__ __launch_bounds__(BLOCK) void k_utf8_count(const wsg_msg* __restrict__ msgs,
                                                      const uint64_t* __restrict__ count, uint32_t msg_room,
                                                      uint64_t msg_cap, uint32_t which,
                                                      const uint64_t* __restrict__ valid,
                                                      unsigned long long* __restrict__ result)
{
    const uint64_t M = min(count[0], uint64_t(msg_room));
    const uint64_t bound = min(msg_cap, count[1]);
    uint64_t invalid = 0, lowest = UINT64_MAX, checked = 0, bytes = 0;
    for (uint64_t m = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; m < M; m += uint64_t(gridDim.x) * BLOCK) {
        const Utf8Rec r = utf8_rec(msgs, uint32_t(m), which);
        if (r.selected && utf8_inside(r, bound)) {
            checked += 1;
            bytes += r.len;
        }
        if (valid[m] < r.len) {
            invalid += 1;
            lowest = min(lowest, m);
        }
    }
    invalid = wave_sum(invalid);
    lowest = wave_min(lowest);
    checked = wave_sum(checked);
    bytes = wave_sum(bytes);
    if ((threadIdx.x & 63) != 0)
        return;
    if (invalid) {
        atomicAdd(result, static_cast<unsigned long long>(invalid));
        atomicMin(result + 1, static_cast<unsigned long long>(lowest));
    }
    if (checked) {
        atomicAdd(result + 2, static_cast<unsigned long long>(checked));
        atomicAdd(result + 3, static_cast<unsigned long long>(bytes));
    }
}

// wsg_utf8_verdicts: d_valid as verdicts wsg_reply_checked takes.  The seed,
// one lane per stream, and, behind a kernel boundary, one lane per record: a
// selected message with d_valid[m] < len fails its stream with 1007 at its
// FIN frame; the stream's first one wins (the verdict word orders by frame).
// Valid traffic issues no atomic.
__global__ __launch_bounds__(BLOCK) void k_utf8_verdict_seed(uint32_t ns, unsigned long long* __restrict__ also)
{
    for (uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; j < ns; j += uint64_t(gridDim.x) * BLOCK)
        also[j] = ~0ull;
}

__global__ __launch_bounds__(BLOCK) void k_utf8_verdicts(const wsg_msg* __restrict__ msgs,
                                                         const uint64_t* __restrict__ count, uint32_t msg_room,
                                                         uint32_t which, const uint64_t* __restrict__ valid,
                                                         uint32_t ns, unsigned long long* __restrict__ also)
{
    const uint64_t M = min(count[0], uint64_t(msg_room));
    for (uint64_t m = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; m < M; m += uint64_t(gridDim.x) * BLOCK) {
        const Utf8Rec r = utf8_rec(msgs, uint32_t(m), which);
        if (!r.selected || valid[m] >= r.len)
            continue;
        const uint64_t* w = reinterpret_cast<const uint64_t*>(msgs + m);
        const uint32_t stream = uint32_t(w[2]), first = uint32_t(w[2] >> 32), nframes = uint32_t(w[3]);
        if (stream < ns)   // (a table that is not this batch's: never a store outside d_also)
            atomicMin(also + stream, uint64_t(WSG_PV_UTF8) | (1007ull << 16) | (uint64_t(first + nframes - 1) << 32));
    }
}

hipError_t launch_utf8_verdicts(hipStream_t s, int rec_grid, int stream_grid, const wsg_msg* msgs,
                                const uint64_t* count, uint32_t msg_room, uint32_t which, const uint64_t* valid,
                                uint32_t n_streams, wsg_proto_verdict* also)
{
    unsigned long long* a = reinterpret_cast<unsigned long long*>(also);
    k_utf8_verdict_seed<<<stream_grid, BLOCK, 0, s>>>(n_streams, a);
    if (msg_room && n_streams)
        k_utf8_verdicts<<<rec_grid, BLOCK, 0, s>>>(msgs, count, msg_room, which, valid, n_streams, a);
    return hipGetLastError();
}

hipError_t launch_utf8_init(hipStream_t s, int grid, const wsg_msg* msgs, const uint64_t* count, uint32_t msg_room,
                            uint64_t* valid, uint64_t* result)
{
    k_utf8_init<<<grid, BLOCK, 0, s>>>(msgs, count, msg_room, valid, result);
    return hipGetLastError();
}

hipError_t launch_utf8_scan(hipStream_t s, int grid, const uint8_t* msg, uint64_t msg_cap, const wsg_msg* msgs,
                            const uint64_t* count, uint32_t msg_room, uint32_t which, uint64_t* valid)
{
    k_utf8_scan<<<grid, BLOCK, 0, s>>>(msg, msg_cap, msgs, count, msg_room, which,
                                       reinterpret_cast<unsigned long long*>(valid));
    return hipGetLastError();
}

hipError_t launch_utf8_count(hipStream_t s, int grid, const wsg_msg* msgs, const uint64_t* count, uint32_t msg_room,
                             uint64_t msg_cap, uint32_t which, const uint64_t* valid, uint64_t* result)
{
    k_utf8_count<<<grid, BLOCK, 0, s>>>(msgs, count, msg_room, msg_cap, which, valid,
                                        reinterpret_cast<unsigned long long*>(result));
    return hipGetLastError();
}

} // namespace wsg
