// wsg_small_frame.h — the small-frame chunk builder, shared by k_encode_small
// (wsg_encode.hip) and the host lane's encode (wsg_lane_device.hip): a send
// descriptor read as dwords, a frame's head (header + close status) and record,
// and the 16-B chunks of a group's wire range ORed together from the frames
// each overlaps.  The payload's blocks come from global memory (the batch
// kernel) or from the lane's LDS copy (StagedBlocks).  Internal linkage, as
// wsg_device.h.
#pragma once

#include "wsg_device.h"

namespace wsg {
namespace {

// A descriptor read as eight dwords: scalar loads cannot fetch the u8 fields
// on gfx9, and a vector load for them would bring an s_waitcnt vmcnt(0)
// that also waits for every data load in flight.
struct Desc {
    uint64_t src_off, len;
    uint32_t key;
    int32_t status;
    uint8_t opcode;
    bool mask;
};

__device__ __forceinline__ Desc load_desc(const wsg_send_desc* d)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(d);
    Desc r;
    r.src_off = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
    r.len = uint64_t(w[2]) | (uint64_t(w[3]) << 32);
    r.key = w[4];
    r.status = int32_t(w[5]);
    r.opcode = uint8_t(w[6]);
    r.mask = ((w[6] >> 8) & 0xFFu) != 0;
    return r;
}
static_assert(offsetof(wsg_send_desc, key) == 16 && offsetof(wsg_send_desc, opcode) == 24 &&
                  offsetof(wsg_send_desc, mask) == 25,
              "wsg_send_desc layout");

// fan_window's blocks for the host lane: the payload's copy staged in LDS.
struct StagedBlocks {
    const v4u* s;          // LDS copy of the aligned blocks from `base` on
    const uint8_t* base;   // 16-B aligned
    __device__ v4u operator()(const uint8_t* p) const { return s[(p - base) >> 4]; }
};

struct SmallFrame {
    uint64_t src;   // offset of the first data byte in the payload arena (an
                    // offset, not an address: loads through a pointer rebuilt
                    // from an integer are flat loads)
    uint32_t key;
    uint32_t geo;   // head bytes (header + status) | header bytes << 8
};

// Bytes [o, o + 16) of a frame of fsize bytes (o < fsize), 0 past its end.
template <class Blocks = GlobalBlocks>
__device__ __forceinline__ v4u small_bytes(const uint8_t* __restrict__ payload, v4u head, const SmallFrame& f,
                                          uint64_t fsize, uint64_t o, Blocks blk = Blocks{})
{
    const uint32_t data0 = f.geo & 0xFFu, hdr = f.geo >> 8;
    v4u out = shr_bytes(head, o);
    const uint64_t lo = o < data0 ? data0 - o : 0;   // chunk bytes [lo, hi) are payload
    const uint64_t hi = fsize - o < CHUNK ? fsize - o : CHUNK;
    if (lo < hi) {
        const v4u w = fan_window(payload + f.src, fsize - data0, int64_t(o) - int64_t(data0), blk);
        out |= (w ^ key_rot(f.key, uint32_t(o - hdr))) & (low_bytes(hi) & ~low_bytes(lo));
    }
    return out;
}

// A frame's head (header bytes + close status, <= 16 bytes: SURVEY Q2/Q3)
// and record for the chunk builder; returns the frame's size.
__device__ __forceinline__ uint64_t small_head(const Desc& d, v4u& h, SmallFrame& fr)
{
    const SendGeom g = send_geom(d.opcode, d.mask, d.len, d.status);
    h = v4u{0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < g.hdr; ++r)
        put_byte(h, r, header_byte(d.opcode, d.mask, g.body, d.key, r));
    if (g.prefix) {   // close status, big-endian, masked like payload bytes 0-1
        put_byte(h, g.hdr, uint32_t((d.status >> 8) & 0xFF) ^ key_byte(d.key, 0));
        put_byte(h, g.hdr + 1, uint32_t(d.status & 0xFF) ^ key_byte(d.key, 1));
    }
    fr = SmallFrame{d.src_off, d.key, (g.hdr + g.prefix) | (g.hdr << 8)};
    return g.hdr + g.body;
}

// The 16-B chunks of a group's wire range [s_off[0], s_off[cnt]) (frames
// 0..cnt-1 of the group, LDS: offsets, heads, records), lanes t, t + nt, ...:
// each chunk ORs together the frames it overlaps; only the range's first and
// last chunk, shared with the neighbouring groups, get byte stores.
template <class Blocks = GlobalBlocks>
__device__ __forceinline__ void small_chunks(const uint8_t* __restrict__ payload, const uint64_t* s_off,
                                             const v4u* s_head, const SmallFrame* s_fr, uint32_t cnt,
                                             uint8_t* __restrict__ wire, uint32_t t, uint32_t nt,
                                             Blocks blk = Blocks{})
{
    const uint64_t r_lo = s_off[0], r_hi = s_off[cnt];
    for (uint64_t p = (r_lo & ~uint64_t(CHUNK - 1)) + uint64_t(t) * CHUNK; p < r_hi; p += uint64_t(nt) * CHUNK) {
        uint32_t a = 0, b = cnt - 1;   // last frame starting at or before p (frame 0 before the range)
        while (a < b) {
            const uint32_t m = (a + b + 1) >> 1;
            if (s_off[m] <= p)
                a = m;
            else
                b = m - 1;
        }
        v4u w = {0, 0, 0, 0};
        for (uint32_t j = a; j < cnt; ++j) {
            const uint64_t off = s_off[j];
            if (off >= p + CHUNK)
                break;
            const uint64_t fsize = s_off[j + 1] - off;
            if (p >= off)
                w |= small_bytes(payload, s_head[j], s_fr[j], fsize, p - off, blk);
            else
                w |= shl_bytes(small_bytes(payload, s_head[j], s_fr[j], fsize, 0, blk), off - p);
        }
        if (p >= r_lo && p + CHUNK <= r_hi) {
            st16nt(wire + p, w);
        } else {
            const uint32_t j0 = p < r_lo ? uint32_t(r_lo - p) : 0;
            const uint32_t j1 = r_hi - p < CHUNK ? uint32_t(r_hi - p) : CHUNK;
            for (uint32_t j = j0; j < j1; ++j)
                wire[p + j] = uint8_t(lane_byte(w, j));
        }
    }
}

} // namespace
} // namespace wsg
