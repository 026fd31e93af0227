// wsg_device.h — device helpers shared by the kernel sources (wsg_decode.hip,
// wsg_encode.hip, wsg_fanout.hip, wsg_lane_device.hip, wsg_misc.hip,
// wsg_messages.hip, wsg_frames.hip, wsg_utf8.hip, wsg_proto.hip, wsg_assembly.hip, wsg_upgrade.hip, wsg_upgrade_client.hip, wsg_carry.hip, wsg_relay.hip): 16-byte loads
// and stores, byte funnels and shifts, the output tile, the frame parse, the block scan, the wave
// reductions, the stream search, a _streams call's span, the error latch and the wsg_msg record codec.  Internal linkage: every source gets its own copy.
#pragma once

#include <type_traits>

#include "wsg_internal.h"

namespace wsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// Streaming loads/stores carry the nontemporal hint (measured faster for
// once-touched data on MI355X: tools/membench.hip); WSG_NT_LOAD/STORE=0
// builds the plain-policy variants for A/B runs.
#ifndef WSG_NT_LOAD
#define WSG_NT_LOAD 1
#endif
#ifndef WSG_NT_STORE
#define WSG_NT_STORE 1
#endif
__device__ __forceinline__ v4u ld16(const uint8_t* p) { return *reinterpret_cast<const v4u*>(p); }
__device__ __forceinline__ v4u ld16nt(const uint8_t* p)
{
    if (WSG_NT_LOAD)
        return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
    return ld16(p);
}
__device__ __forceinline__ void st16nt(uint8_t* p, v4u v)
{
    if (WSG_NT_STORE)
        __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(p));
    else
        *reinterpret_cast<v4u*>(p) = v;
}

__device__ __forceinline__ uint32_t ab(uint32_t hi, uint32_t lo, uint32_t b)
{
    return __builtin_amdgcn_alignbyte(hi, lo, b);   // ({hi,lo} >> 8b)[31:0]
}

// Bytes [s, s+16) of the 32-byte little-endian window lo:hi (v_alignbyte_b32).
__device__ __forceinline__ v4u funnel(v4u lo, v4u hi, uint32_t s)
{
    const uint32_t b = s & 3u;
    v4u r;
    switch (s >> 2) {
    case 0:
        r = v4u{ab(lo.y, lo.x, b), ab(lo.z, lo.y, b), ab(lo.w, lo.z, b), ab(hi.x, lo.w, b)};
        break;
    case 1:
        r = v4u{ab(lo.z, lo.y, b), ab(lo.w, lo.z, b), ab(hi.x, lo.w, b), ab(hi.y, hi.x, b)};
        break;
    case 2:
        r = v4u{ab(lo.w, lo.z, b), ab(hi.x, lo.w, b), ab(hi.y, hi.x, b), ab(hi.z, hi.y, b)};
        break;
    default:
        r = v4u{ab(hi.x, lo.w, b), ab(hi.y, hi.x, b), ab(hi.z, hi.y, b), ab(hi.w, hi.z, b)};
        break;
    }
    return r;
}

// 128-bit byte shifts and byte masks (runtime counts) built on funnel().
__device__ __forceinline__ v4u shr_bytes(v4u x, uint64_t o)   // byte j = x[j + o]
{
    return o >= CHUNK ? v4u{0, 0, 0, 0} : funnel(x, v4u{0, 0, 0, 0}, uint32_t(o));
}
__device__ __forceinline__ v4u shl_bytes(v4u x, uint64_t s)   // byte j = x[j - s]
{
    return s == 0 ? x : s >= CHUNK ? v4u{0, 0, 0, 0} : funnel(v4u{0, 0, 0, 0}, x, uint32_t(CHUNK - s));
}
__device__ __forceinline__ v4u low_bytes(uint64_t n)   // bytes [0, n) = 0xFF
{
    const uint64_t lo = n >= 8 ? ~uint64_t(0) : (uint64_t(1) << (8 * n)) - 1;
    const uint64_t hi = n >= 16 ? ~uint64_t(0) : n <= 8 ? 0 : (uint64_t(1) << (8 * (n - 8))) - 1;
    return v4u{uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32)};
}

// Stores of a once-written output stream.  Write-through (sc1) buffer stores
// beat nontemporal ones in tools/membench.hip's copy (C2 footprint: 83.4-83.9
// vs 85.0-85.5 us) and write-only stream (43.6 vs 47.4 us), but NOT in
// k_decode: 90.7 vs 87.9 us on C2 and 0.825 vs 0.782 ms on C3's ragged
// frames, and 90.1 vs 86.3 us with buffer loads too (tools/tune.py, same box,
// interleaved, two boxes), so decode keeps nontemporal stores; the fan-out
// (write-only) takes them.  WSG_OUT_SC1=1 builds the decode variant for A/B.
#ifndef WSG_OUT_SC1
#define WSG_OUT_SC1 0
#endif
#ifndef WSG_OUT_AUX
#define WSG_OUT_AUX 16   // cache-policy bits of the write-through stores (16 = sc1, 17 = sc0 | sc1; A/B)
#endif
struct OutTile {
    uint8_t* p;   // tile base (wave-uniform)
    bool sc1;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ OutTile(uint8_t* base, uint32_t bytes, bool write_through = WSG_OUT_SC1 != 0)
        : p(base), sc1(write_through)
    {
        if (sc1)
            rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
    }
    // whole 16-B chunk at tile offset o (o + 16 <= bytes)
    __device__ __forceinline__ void put(uint32_t o, v4u v) const
    {
        if (sc1)
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, o, 0, WSG_OUT_AUX);
        else
            st16nt(p + o, v);
    }
};

// Byte j (runtime) of a 16-byte value, through two 64-bit halves so that no
// register array is indexed at run time (that would spill to scratch).
__device__ __forceinline__ uint32_t lane_byte(v4u v, uint32_t j)
{
    const uint64_t lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
    const uint64_t hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
    return uint32_t((j < 8 ? lo >> (8u * j) : hi >> (8u * (j - 8))) & 0xFFu);
}

__device__ __forceinline__ void put_byte(v4u& w, uint32_t j, uint32_t b)
{
    const uint64_t m = uint64_t(b & 0xFFu) << (8u * (j & 7u));
    const uint64_t lo = j < 8 ? m : 0, hi = j < 8 ? 0 : m;
    w.x |= uint32_t(lo);
    w.y |= uint32_t(lo >> 32);
    w.z |= uint32_t(hi);
    w.w |= uint32_t(hi >> 32);
}

__device__ __forceinline__ uint64_t lane_bcast(uint64_t v, int src)
{
    const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(v), src);
    const uint32_t hi = __builtin_amdgcn_readlane(uint32_t(v >> 32), src);
    return uint64_t(lo) | (uint64_t(hi) << 32);
}

__device__ __forceinline__ uint32_t wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// A wave-uniform value computed by vector instructions, moved to SGPRs.
__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// (the builtins return int: each half goes through uint32_t, else a low half
// of 2^31 or more sign-extends over the high one)
__device__ __forceinline__ uint64_t uni(uint64_t x)
{
    return uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(x)))) |
           (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(x >> 32)))) << 32);
}

// Bytes [0, n) of an 8-byte word as a mask.
__device__ __forceinline__ uint64_t bytes_below(int64_t n)
{
    return n <= 0 ? 0ull : n >= 8 ? ~0ull : (1ull << (8 * n)) - 1ull;
}

__device__ __forceinline__ uint32_t lane_bcast32(uint32_t v, uint32_t src)
{
    return uint32_t(__builtin_amdgcn_readlane(v, int(uni(src))));
}

// One stream of a _streams call (wave-uniform).
struct SpanIn {
    uint64_t off, len;
    bool ok;
};

// Span j as given and whether it may be walked: inside the wire, and not
// starting before the end of span j - 1 where that one lies inside the wire.
__device__ __forceinline__ SpanIn span_in(const wsg_stream_span* span, uint32_t j, uint64_t wire_len)
{
    static_assert(sizeof(wsg_stream_span) == 32 && offsetof(wsg_stream_span, consumed) == 16, "wsg_stream_span layout");
    const uint64_t* w = reinterpret_cast<const uint64_t*>(span + j);
    SpanIn s;
    s.off = uni(w[0]);
    s.len = uni(w[1]);
    bool ok = s.off <= wire_len && s.len <= wire_len - s.off;
    if (ok && j > 0) {
        const uint64_t* p = reinterpret_cast<const uint64_t*>(span + (j - 1));
        const uint64_t poff = uni(p[0]), plen = uni(p[1]);
        if (poff <= wire_len && plen <= wire_len - poff && s.off < poff + plen)
            ok = false;
    }
    s.ok = uni(uint32_t(ok)) != 0;
    return s;
}

// Span j as span_in judges it, for a lane of its own (span_in's values are
// the wave's): off, len, consumed and whether the span may be walked.
struct SpanLane {
    uint64_t off, len, consumed;
    bool ok;
};

__device__ __forceinline__ SpanLane span_in_lane(const wsg_stream_span* span, uint64_t j, uint64_t wire_len)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(span + j);
    SpanLane s;
    s.off = w[0];
    s.len = w[1];
    s.consumed = w[2];
    s.ok = s.off <= wire_len && s.len <= wire_len - s.off;
    if (s.ok && j > 0) {
        const uint64_t* p = reinterpret_cast<const uint64_t*>(span + (j - 1));
        const uint64_t poff = p[0], plen = p[1];
        if (poff <= wire_len && plen <= wire_len - poff && s.off < poff + plen)
            s.ok = false;
    }
    return s;
}

// Bytes [0, k) of a dword as a mask (k <= 0: none, k >= 4: all).
__device__ __forceinline__ uint32_t low_bytes(int k)
{
    return k <= 0 ? 0u : k >= 4 ? ~0u : (1u << (8 * k)) - 1u;
}

// Frame [s, limit) as PrepareReceiveFrame parses it when delivered whole
// (ws.cpp:320-386), with the batch checks of wsg_decode_batch.  Returns 0 or
// the frame's error; on error r describes an empty payload at s, so the
// frame's bytes are copied.
// (Block16: the aligned 16-byte block at a wire offset; global memory here,
// LDS for the host lane's staged wire.)
template <class Block16>
__device__ __forceinline__ int frame_parse_b(Block16 block, uint64_t wire_len, uint64_t s, uint64_t limit,
                                             wsg_recv_info& r)
{
    r = wsg_recv_info{};
    int e = WSG_ETRUNC;
    if (s < wire_len) {
        const uint64_t avail = wire_len - s;
        // wire[s .. s+16) as two u64 from the aligned 32-byte window, with
        // 64-bit shifts only (scalar instructions when s is wave-uniform)
        const uint64_t a0 = s & ~uint64_t(15);
        const v4u lo = block(a0);
        const v4u hi = (a0 + 16 < wire_len) ? block(a0 + 16) : v4u{0, 0, 0, 0};
        uint64_t q0 = uint64_t(lo.x) | (uint64_t(lo.y) << 32), q1 = uint64_t(lo.z) | (uint64_t(lo.w) << 32);
        const uint64_t q2 = uint64_t(hi.x) | (uint64_t(hi.y) << 32), q3 = uint64_t(hi.z) | (uint64_t(hi.w) << 32);
        uint64_t q2s = q2;
        if (s & 8) {
            q0 = q1;
            q1 = q2;
            q2s = q3;
        }
        const uint32_t b = 8u * uint32_t(s & 7);
        const uint64_t h0 = b ? (q0 >> b) | (q1 << (64u - b)) : q0;
        const uint64_t h1 = b ? (q1 >> b) | (q2s << (64u - b)) : q1;
        e = parse_header([&](uint32_t k) { return uint8_t(k < 8 ? h0 >> (8u * k) : h1 >> (8u * (k - 8))); }, avail, r);
        if (e == 0) {
            if (r.len > avail - r.hdr_len)
                e = WSG_ETRUNC;
            else if (limit < s || limit - s < r.hdr_len || r.len > limit - s - r.hdr_len)
                e = WSG_EINVAL;   // the next frame starts inside this one
        }
    }
    if (e != 0) {
        r = wsg_recv_info{};
        r.payload_off = s;
        r.error = int8_t(e);
    } else {
        r.payload_off = s + r.hdr_len;
    }
    return e;
}

__device__ __forceinline__ int frame_parse(const uint8_t* __restrict__ wire, uint64_t wire_len, uint64_t s,
                                           uint64_t limit, wsg_recv_info& r)
{
    return frame_parse_b([wire](uint64_t a) { return ld16(wire + a); }, wire_len, s, limit, r);
}

// wsg_recv_info as four 8-byte words (a struct store of the byte fields went
// through scratch).
__device__ __forceinline__ void store_info(wsg_recv_info* dst, const wsg_recv_info& r)
{
    static_assert(offsetof(wsg_recv_info, key) == 16 && offsetof(wsg_recv_info, opcode) == 20 &&
                      offsetof(wsg_recv_info, b0) == 24 && offsetof(wsg_recv_info, error) == 25 &&
                      sizeof(wsg_recv_info) == 32,
                  "wsg_recv_info layout");
    uint64_t* w = reinterpret_cast<uint64_t*>(dst);
    w[0] = r.payload_off;
    w[1] = r.len;
    w[2] = uint64_t(r.key) | (uint64_t(r.opcode) << 32) | (uint64_t(r.fin) << 40) | (uint64_t(r.masked) << 48) |
           (uint64_t(r.hdr_len) << 56);
    w[3] = uint64_t(r.b0) | (uint64_t(uint8_t(r.error)) << 8);
}

// Everything a piece needs about its frame (wave-uniform).
struct FrameRec {
    uint64_t off;       // wire offset of the frame
    uint64_t pw;        // wire offset of the payload (status prefix included)
    uint64_t data_w;    // wire offset of the first data byte
    uint64_t end;       // wire offset one past the frame
    const uint8_t* src; // data bytes
    uint64_t body;
    uint32_t key;
    uint32_t hdr;
    uint32_t prefix;
    int32_t status;
    uint8_t opcode;
    bool mask;
};

__device__ __forceinline__ FrameRec make_rec(uint64_t off, const uint8_t* src, uint64_t len, uint32_t key,
                                             int32_t status, uint8_t opcode, bool mask)
{
    const SendGeom g = send_geom(opcode, mask, len, status);
    FrameRec r;
    r.off = off;
    r.pw = off + g.hdr;
    r.data_w = r.pw + g.prefix;
    r.end = r.pw + g.body;
    r.src = src;
    r.body = g.body;
    r.key = key;
    r.hdr = g.hdr;
    r.prefix = g.prefix;
    r.status = status;
    r.opcode = opcode;
    r.mask = mask;
    return r;
}

// 16 payload bytes as seen from a chunk: byte j = payload[c + j] where that
// offset is inside [0, len) (else 0).  Reads only aligned 16-B blocks that
// hold a wanted byte, at most two.
// The 16-B block at an aligned address: a global load, or (the lane) the
// block's copy staged in LDS.
struct GlobalBlocks {
    __device__ v4u operator()(const uint8_t* p) const { return ld16(p); }
};

template <class Blocks = GlobalBlocks>
__device__ __forceinline__ v4u fan_window(const uint8_t* __restrict__ payload, uint64_t len, int64_t c,
                                          Blocks blk = Blocks{})
{
    // offsets relative to `payload`, loads through pointer arithmetic on it
    // (global_* loads; a pointer rebuilt from an integer loads flat_*)
    const uint32_t s = uint32_t((reinterpret_cast<uintptr_t>(payload) + uint64_t(c)) & 15u);
    const int64_t r0 = c - int64_t(s);   // aligned block holding byte c, relative to payload
    const int64_t n = int64_t(len);
    v4u lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (r0 < n && r0 + 16 > 0)
        lo = blk(payload + r0);
    if (s != 0 && r0 + 16 < n && r0 + 32 > 0)
        hi = blk(payload + r0 + 16);
    return s ? funnel(lo, hi, s) : lo;
}

// Header + close-status bytes of frame R (<= 16, as PrepareSendFrame writes
// them, the status masked like payload bytes 0-1: SURVEY Q2/Q3), zero past
// them; wave-uniform.
__device__ __forceinline__ v4u frame_head(const FrameRec& R)
{
    v4u h = {0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < R.hdr; ++r)
        put_byte(h, r, header_byte(R.opcode, R.mask, R.body, R.key, r));
    if (R.prefix) {
        put_byte(h, R.hdr, uint32_t((R.status >> 8) & 0xFF) ^ key_byte(R.key, 0));
        put_byte(h, R.hdr + 1, uint32_t(R.status & 0xFF) ^ key_byte(R.key, 1));
    }
    return h;
}

// ---- block scan (wave64) ----------------------------------------------------
struct OpAdd {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Exclusive scan over the block under op (identity 0); *total = op over the
// block.  The inclusive value is op(result, v).
template <class T, class Op>
__device__ T block_scan_ex(T v, Op op, T* total)
{
    __shared__ T wsum[BLOCK / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(inc, d, 64);
        if (lane >= d)
            inc = op(u, inc);
    }
    // exclusive within the wave: the lane before's inclusive value, which a sum gives without
    // that shuffle (10.4 against 10.0 us in k_encode_scan_local<false> at 1 Mi frames, profiles/r11)
    T ex = inc - v;
    if (!std::is_same<Op, OpAdd>::value) {
        ex = __shfl_up(inc, 1, 64);
        ex = lane ? ex : T(0);
    }
    if (lane == 63)
        wsum[wid] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) {
        if (k < wid)
            before = op(before, wsum[k]);
        all = op(all, wsum[k]);
    }
    __syncthreads();
    *total = all;
    return op(before, ex);
}

// One block scans the block partials in[0..nb) under op, BLOCK of them a pass,
// carrying the running value: the exclusive prefixes to pre (null: none
// wanted), the total returned.  Called by every lane of a BLOCK-thread block.
template <class T, class Op>
__device__ __forceinline__ T scan_partials(const T* __restrict__ in, T* __restrict__ pre, uint32_t nb, Op op)
{
    T carry = 0;
    for (uint32_t c = 0; c < nb; c += BLOCK) {
        const uint32_t b = c + threadIdx.x;
        T tot;
        const T ex = block_scan_ex(b < nb ? in[b] : T(0), op, &tot);
        if (pre && b < nb)
            pre[b] = op(carry, ex);
        carry = op(carry, tot);
    }
    return carry;
}

// Sum and minimum over the wave, in lane 0.
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_down(v, d, 64);
    return v;   // lane 0
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t u = __shfl_down(v, d, 64);
        v = u < v ? u : v;
    }
    return v;   // lane 0
}

// Last j < ns with sf[j] <= i (0 when there is none): the stream of frame i
// (an empty stream shares its first index with the next one, which wins).
__device__ __forceinline__ uint32_t stream_of(const uint32_t* __restrict__ sf, uint32_t ns, uint32_t i)
{
    uint32_t lo = 0, hi = ns;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sf[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Last j in [lo, hi) with off[j] <= p (lo when there is none): stream_of over
// 64-bit offsets and a range of streams (an empty stream shares its offset
// with the next one, which wins).
__device__ __forceinline__ uint32_t stream_of64(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t p)
{
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// stream_of64 by the whole wave, every argument and the result wave-uniform
// (off[lo] <= p): lane i probes the i-th of 64 evenly spaced entries and a
// ballot picks the interval, so 4096 streams take two dependent loads and
// 2^18 three, where the binary search takes twelve and eighteen.
__device__ __forceinline__ uint32_t stream_of64_wave(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi,
                                                     uint64_t p, uint32_t lane)
{
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + 63) / 64;
        const uint64_t at = uint64_t(lo) + uint64_t(lane) * step;
        const bool le = at < hi && off[at] <= p;   // true in lanes 0..k-1: off does not decrease
        const uint32_t k = max(uint32_t(__builtin_popcountll(__ballot(le))), 1u);
        lo = uni(lo + (k - 1) * step);
        hi = min(lo + step, hi);
    }
    return lo;
}

// The error latch wsg_sync decodes: the smallest (index << 8 | -code) wins,
// so the first failing frame (or span) does, whatever the kernels' order.
__device__ __forceinline__ void latch(unsigned long long* err, uint64_t index, int code)
{
    atomicMin(err, (static_cast<unsigned long long>(index) << 8) | static_cast<unsigned long long>(-code));
}

// [lo, hi) of a frame's pieces, `before` and `after` the piece counts in front
// of the frame and of the next one, clamped to the cap records there are.
__device__ __forceinline__ void piece_range(uint64_t before, uint64_t after, uint64_t cap, uint64_t& lo, uint64_t& hi)
{
    lo = min(before, cap);
    hi = max(min(after, cap), lo);
}

// ---- wsg_msg as five 8-byte words --------------------------------------------
static_assert(sizeof(wsg_msg) == 40 && offsetof(wsg_msg, len) == 8 && offsetof(wsg_msg, stream) == 16 &&
                  offsetof(wsg_msg, nframes) == 24 && offsetof(wsg_msg, status) == 28 &&
                  offsetof(wsg_msg, kind) == 32 && offsetof(wsg_msg, opcode) == 33,
              "wsg_msg layout");
// The record's fields in registers (first: the message's first frame).
struct MsgRec {
    uint64_t off, len;
    uint32_t stream, first, kind, op;
    int32_t status;
};

__device__ __forceinline__ void put_msg(wsg_msg* m, const MsgRec& r, uint32_t last)   // last: the FIN frame
{
    uint64_t* w = reinterpret_cast<uint64_t*>(m);
    w[0] = r.off;
    w[1] = r.len;
    w[2] = uint64_t(r.stream) | (uint64_t(r.first) << 32);
    w[3] = uint64_t(last - r.first + 1) | (uint64_t(uint32_t(r.status)) << 32);
    w[4] = uint64_t(r.kind) | (uint64_t(r.op) << 8);
}

__device__ __forceinline__ MsgRec get_msg(const wsg_msg* __restrict__ m)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(m);
    return MsgRec{w[0], w[1], uint32_t(w[2]), uint32_t(w[2] >> 32), uint32_t(w[4]) & 0xFFu,
                  (uint32_t(w[4]) >> 8) & 0xFFu, int32_t(w[3] >> 32)};
}

// off + len, saturating
__device__ __forceinline__ uint64_t msg_end(uint64_t off, uint64_t len)
{
    return off + len < off ? UINT64_MAX : off + len;
}
__device__ __forceinline__ uint64_t msg_end(const wsg_msg* __restrict__ msgs, uint64_t m)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(msgs + m);
    return msg_end(w[0], w[1]);
}

} // namespace

// Typed arrays carved back to back out of one block, each start rounded up
// to `align` bytes from the end of the array before it.
struct Carve {
    uint8_t* base;
    uint64_t align;
    uint64_t at = 0;
    template <class T>
    T* take(uint64_t count)
    {
        T* p = reinterpret_cast<T*>(base + at);
        at += (count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
};

} // namespace wsg
