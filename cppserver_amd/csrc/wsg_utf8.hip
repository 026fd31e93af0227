// wsg_utf8.hip — UTF-8 validation of decoded messages (wsg_check_utf8) and of
// messages read where they lie in the masked wire (wsg_check_utf8_wire).
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

// ---- UTF-8 from the masked wire (wsg_check_utf8_wire) -------------------------
// The same rule with no d_msg: the message plan's piece records (k_msg_finalize:
// one frame's payload offset, dense offset, length and key, in dense order) say
// where every message byte sits in the wire and under which key.  A record's
// k is read here as the k-th 4 KiB of the WIRE from the 128-byte line of the
// payload's first byte, which needs no more records than the dense cut the
// plan counted (poff mod 128 <= 127), leaves at most one record of a frame
// empty, and makes every chunk of a wave an aligned 16-byte block of d_wire.
struct WirePiece {
    uint64_t ws, we;   // its payload bytes: wire [ws, we); ws >= we: none.  Its first row: ws & ~(PIECE_ALIGN - 1)
    uint64_t delta;    // dense position of wire byte x: x + delta (mod 2^64)
    uint32_t key;      // the frame's key at wire phase: byte x is masked with key byte x mod 4
};

__device__ __forceinline__ WirePiece utf8_wire_piece(const MsgPiece* __restrict__ rec, uint64_t wire_len)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(rec);
    const uint64_t poff = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
    const uint64_t d0 = uint64_t(w[2]) | (uint64_t(w[3]) << 32);
    const uint64_t len = uint64_t(w[4]) | (uint64_t(w[5]) << 32);
    const uint64_t lo = (poff & ~(PIECE_ALIGN - 1)) + uint64_t(w[7]) * PIECE;
    const uint64_t end = poff + len;
    WirePiece p;
    p.delta = d0 - poff;
    p.key = key_rot(w[6], 0u - uint32_t(poff));   // payload byte i lies at wire offset poff + i
    p.ws = max(lo, poff);
    p.we = min(lo + PIECE, end);
    if (end < poff || end > wire_len)   // (not a frame of this wire: never a read outside it)
        p.ws = p.we = 0;
    return p;
}

// The up-to-3 message bytes in front of piece q's first byte, unmasked, as the
// dword of the positions -4..-1 (00 where there is none): they lie in the
// records before q, one frame and key each, however many empty, failed or
// control frames the wire holds between them.  A frame has at most one empty
// record and every other record holds a byte, so six records always suffice.
__device__ __forceinline__ uint32_t utf8_wire_before(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                     const MsgPiece* __restrict__ recs, uint64_t q)
{
    uint32_t h = 0, got = 0;
    for (uint32_t step = 0; step < 8 && q > 0 && got < 3; ++step) {
        const WirePiece P = utf8_wire_piece(recs + --q, wire_len);
        for (uint64_t p = P.we; p > P.ws && got < 3; ++got) {
            --p;
            h |= (uint32_t(wire[p]) ^ key_byte(P.key, p)) << (8u * (3u - got));
        }
    }
    return h;
}

// ... and behind its last byte: the dword of the positions 0..3 from there.
__device__ __forceinline__ uint32_t utf8_wire_after(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                    const MsgPiece* __restrict__ recs, uint64_t q, uint64_t pieces)
{
    uint32_t t = 0, got = 0;
    for (uint32_t step = 0; step < 8 && q + 1 < pieces && got < 3; ++step) {
        const WirePiece P = utf8_wire_piece(recs + ++q, wire_len);
        for (uint64_t p = P.ws; p < P.we && got < 3; ++p, ++got)
            t |= (uint32_t(wire[p]) ^ key_byte(P.key, p)) << (8u * got);
    }
    return t;
}

// d[0..6) is the window -4..19 of a chunk; h holds 4 bytes for the window
// indices [wi, wi + 4) (wi in (-4, 24); the window is 00 where h has a byte).
__device__ __forceinline__ void utf8_window_or(uint32_t d[6], int wi, uint32_t h)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int s = wi - 4 * k;
        if (s > -4 && s < 4)
            d[k] |= s >= 0 ? h << (8 * s) : h >> (8 * -s);
    }
}

// Bit i: byte i of the chunk is >= 0x80.  (Bit 7 of a dword's four bytes
// gathered by one multiplication: the sixteen partial products meet nowhere.)
__device__ __forceinline__ uint32_t utf8_chunk_high(v4u c)
{
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        bits |= ((((c[k] >> 7) & 0x01010101u) * 0x01020408u) >> 24 & 0xFu) << (4 * k);
    return bits;
}

// Row u (wave-uniform, run time) of a piece's chunks, by selects: the rows stay in registers.
__device__ __forceinline__ v4u utf8_row(const v4u (&c)[EU], uint32_t u)
{
    v4u r = c[0];
#pragma unroll
    for (int k = 1; k < EU; ++k)
        r = u == uint32_t(k) ? c[k] : r;
    return r;
}

// Bits [x, 16) of a chunk's 16 positions.
__device__ __forceinline__ uint32_t utf8_bits_from(int64_t x)
{
    return x <= 0 ? 0xFFFFu : x >= 16 ? 0u : (0xFFFFu << uint32_t(x)) & 0xFFFFu;
}

} // namespace

// One wave per piece record (grid-stride), EU rows of 64 aligned 16-byte
// chunks: one nontemporal load each, XOR with the key at the chunk's payload
// phase (wave-uniform: chunks are 16 apart), the bytes outside the piece's
// payload cleared in the two chunks that hold its ends.  No byte >= 0x80 in
// the wave: done.  Otherwise one search of d_msgs finds the one message the
// piece's frame belongs to (a close message's checked range starts 2 bytes
// into its buffer: the window's bounds see to that); a piece of an unselected
// message is done.  The 4 bytes either side of a chunk come from the
// neighbouring lanes' and rows' registers, and the 3 on either side of the
// piece from the neighbouring records, fetched only where the message goes on
// beyond the piece and a byte >= 0x80 lies within 3 bytes of that end.  Only
// the piece's own positions are judged.
__global__ __launch_bounds__(BLOCK) void k_utf8_wire(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                     const uint64_t* __restrict__ tot,
                                                     const MsgPiece* __restrict__ piece_recs, uint64_t pieces_cap,
                                                     const wsg_msg* __restrict__ msgs,
                                                     const uint64_t* __restrict__ count, uint32_t msg_room,
                                                     uint32_t which, unsigned long long* __restrict__ valid)
{
    const uint32_t M = uint32_t(min(count[0], uint64_t(msg_room)));
    if (M == 0)
        return;
    const uint32_t waves = gridDim.x * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t pieces = uint32_t(min(min(tot[3], pieces_cap), uint64_t(UINT32_MAX)));   // (the host's bound fits a word)
    // (wave-uniform loop: every lane of a wave takes part in the shuffles)
    for (uint64_t q = uint64_t(blockIdx.x) * (BLOCK / 64) + wave_id(); q < pieces; q += waves) {
        const WirePiece P = utf8_wire_piece(piece_recs + q, wire_len);
        if (P.ws >= P.we)
            continue;   // piece counts are an upper bound
        const uint64_t row0 = P.ws & ~(PIECE_ALIGN - 1);
        const uint32_t kw = P.key;   // (every chunk starts at a wire offset that is 0 mod 4)
        v4u c[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t a = row0 + (uint64_t(u) * 64 + lane) * CHUNK;
            c[u] = a < P.we && a + CHUNK > P.ws ? ld16nt(wire + a) : v4u{0, 0, 0, 0};
        }
        uint32_t hot = 0;
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t a = row0 + (uint64_t(u) * 64 + lane) * CHUNK;
            const bool in = a < P.we && a + CHUNK > P.ws;
            c[u] = in ? c[u] ^ kw : c[u];
            if (in && (a < P.ws || a + CHUNK > P.we)) {   // a chunk shared with the header or the next frame
                const int lo = a < P.ws ? int(P.ws - a) : 0, hi = P.we - a < CHUNK ? int(P.we - a) : int(CHUNK);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    c[u][k] &= low_bytes(hi - 4 * k) & ~low_bytes(lo - 4 * k);
            }
            hot |= uint32_t(((c[u].x | c[u].y | c[u].z | c[u].w) & UTF8_H) != 0) << u;   // a bad position is never an ASCII byte
        }
        if (__ballot(hot != 0) == 0)
            continue;
        const uint64_t dlo = P.ws + P.delta, dhi = P.we + P.delta;   // the piece in the dense layout
        const uint32_t m = uni(utf8_first_beyond_wave(msgs, 0, M, dlo));
        if (m >= M)
            continue;
        const Utf8Rec r = utf8_rec(msgs, m, which);
        if (!r.selected)
            continue;
        // a byte >= 0x80 among the piece's first / last 3 bytes, with message bytes beyond that end
        uint32_t near_head = 0, near_tail = 0;
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t a = row0 + (uint64_t(u) * 64 + lane) * CHUNK;
            const int64_t wh = int64_t(P.ws - a), wt = int64_t(P.we - a);
            const uint32_t bytes = utf8_chunk_high(c[u]);
            near_head |= bytes & utf8_bits_from(wh) & ~utf8_bits_from(wh + 3);
            near_tail |= bytes & utf8_bits_from(wt - 3) & ~utf8_bits_from(wt);
        }
        uint32_t head = 0, tail = 0;
        if (dlo > r.off && __ballot(near_head != 0) != 0)
            head = utf8_wire_before(wire, wire_len, piece_recs, q);
        if (dhi < r.end && __ballot(near_tail != 0) != 0)
            tail = utf8_wire_after(wire, wire_len, piece_recs, q, pieces);
        // (one copy of the rule's code: the row in hand picked out of the registers by selects)
#pragma unroll 1
        for (uint32_t u = 0; u < uint32_t(EU); ++u) {
            if (__ballot((hot >> u) & 1u) == 0)
                continue;
            const v4u cu = utf8_row(c, u);
            uint32_t pre = uint32_t(__shfl_up(cu.w, 1, 64)), post = uint32_t(__shfl_down(cu.x, 1, 64));
            const uint32_t row_before = u ? uint32_t(__builtin_amdgcn_readlane(utf8_row(c, u - 1).w, 63)) : 0u;
            const uint32_t row_after = u + 1 < uint32_t(EU) ? uint32_t(__builtin_amdgcn_readlane(utf8_row(c, u + 1).x, 0)) : 0u;
            pre = lane == 0 ? row_before : pre;
            post = lane == 63 ? row_after : post;
            if (!((hot >> u) & 1u))
                continue;
            const uint64_t a = row0 + (uint64_t(u) * 64 + lane) * CHUNK;
            const int64_t wh = int64_t(P.ws - a), wt = int64_t(P.we - a);   // the piece's ends, from the chunk
            uint32_t d[6] = {pre, cu.x, cu.y, cu.z, cu.w, post};
            if (head && wh > -4 && wh < 24)
                utf8_window_or(d, int(wh), head);            // positions ws - 4 .. ws - 1
            if (tail && wt > -8 && wt < 20)
                utf8_window_or(d, int(wt) + 4, tail);        // positions we .. we + 3
            const uint64_t pd = a + P.delta;   // dense position of the chunk's byte 0 (mod 2^64 in front of the payload)
            const int64_t ro = int64_t(r.off - pd), re = int64_t(r.end - pd);
            const int lo = ro < -4 ? -4 : ro > 20 ? 20 : int(ro), hi = re < -4 ? -4 : re > 20 ? 20 : int(re);
            // (only the piece's own positions: the context bytes are judged by their own waves)
            const uint32_t bad = utf8_chunk_bad(d[0], v4u{d[1], d[2], d[3], d[4]}, d[5], lo, hi) & utf8_bits_from(wh) &
                                 ~utf8_bits_from(wt);
            if (bad)
                atomicMin(valid + m, static_cast<unsigned long long>(pd + uint32_t(__builtin_ctz(bad)) - r.off));
        }
    }
}

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

// wsg_reply_validated: the seed of its verdict scratch, one lane per stream:
// the caller's d_also[j] where it is given, is not all 0xFF and names a frame
// of stream j, all 0xFF otherwise, so that an entry k_proto_merge would
// ignore never stands below a UTF-8 verdict in k_utf8_verdicts' minimum.
__global__ __launch_bounds__(BLOCK) void k_utf8_also_seed(uint32_t n, const uint32_t* __restrict__ sf, uint32_t ns,
                                                          const uint64_t* __restrict__ also_in,
                                                          unsigned long long* __restrict__ also)
{
    for (uint64_t j = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; j < ns; j += uint64_t(gridDim.x) * BLOCK) {
        uint64_t a = also_in ? also_in[j] : UINT64_MAX;
        const uint32_t frame = uint32_t(a >> 32);
        const uint32_t start = min(sf[j], n), end = max(min(sf[j + 1], n), start);
        if (frame < start || frame >= end)
            a = UINT64_MAX;
        also[j] = a;
    }
}

hipError_t launch_utf8_verdicts_over(hipStream_t s, int stream_grid, const Batch& b,
                                     const wsg_proto_verdict* also_in, const MsgOut& o, const Utf8Inside& u)
{
    unsigned long long* a = reinterpret_cast<unsigned long long*>(u.also);
    k_utf8_also_seed<<<stream_grid, BLOCK, 0, s>>>(b.n, b.stream_first, b.n_streams,
                                                   reinterpret_cast<const uint64_t*>(also_in), a);
    if (b.n && b.n_streams && u.which)
        k_utf8_verdicts<<<u.rec_grid, BLOCK, 0, s>>>(o.msgs, o.count, b.n, u.which, u.valid, b.n_streams, a);
    return hipGetLastError();
}

hipError_t launch_utf8_wire(hipStream_t s, int grid, const Batch& b, const MsgOut& o, const MsgScratch& x,
                            uint32_t which, uint64_t* valid)
{
    k_utf8_wire<<<grid, BLOCK, 0, s>>>(b.wire, b.wire_len, x.plans.ref.tot, x.pieces, x.pieces_cap, o.msgs, o.count,
                                       b.n, which, reinterpret_cast<unsigned long long*>(valid));
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
