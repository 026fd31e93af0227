// wsg_fanout.hip — fan-out encode on gfx950 (CDNA4): one payload framed k
// times, the frames differing only in their mask key (wsg_fanout_encode,
// wsg_fanout_encode_many; the ws_multicast tick).  Write-only: every output
// byte is written exactly once, whole 16-byte chunks.
//   k_fanout_period - frame sizes that are a multiple of 4 (launch_fanout_period):
//                     a lane builds its chunk's template once and then only
//                     stores, pass after pass;
//   k_fanout_flat   - every other frame size (launch_fanout): the k frames as
//                     one byte stream, streaming waves plus edge blocks.
#include "wsg_device.h"

namespace wsg {

namespace {

#ifndef WSG_DIAG_FAN
#define WSG_DIAG_FAN 0   // timing-only fan-out diagnostics: 1 no key loads, 2 no payload loads, 4 stores only, 8 no edge blocks; period path: 16 no template loads, 32 no key loads, 64 no stores, 128 prologue only, 256 empty
#endif
#ifndef WSG_FAN_PERIOD
#define WSG_FAN_PERIOD 1   // fan-out: period path (k_fanout_period) where the frame size allows; 0 = flat kernel only
#endif
#ifndef WSG_FAN_UNROLL
#define WSG_FAN_UNROLL 1   // fan-out period path: passes per loop iteration (A/B)
#endif
constexpr int FAN_UNROLL = WSG_FAN_UNROLL;   // (a constant: a macro in a pragma is not expanded when the asm target compiles the preprocessed source)
// Fan-out period path, many messages per launch (wsg_fanout_encode_many, the
// ws_multicast tick).  Round 5 capped the launch at 4 resident one-wave
// workgroups per CU (a dynamic LDS reserve the kernel does not use) with the
// single message's ~6 waves per CU per message: 16 x C4 in 111-113 us, 0.86-0.88
// of the runtime's fill of the same bytes (97 us).  Uncapped (register-limited
// residency) with ~46 waves per CU per message — 23 x Q = 11799 waves for
// C4, each 3-4 passes — it is 100.7-104 us, 0.93-0.97 of the fill; fewer or more
// waves lose it on both sides (24: 121 us, 36: 117, 56: 113, 64: 124, 96: 169,
// where one-wave workgroups come faster than the dispatcher launches them),
// and so does the cap at these counts (profiles/r6/fan_*_ab*.log).
#ifndef WSG_FAN_CAP
#define WSG_FAN_CAP 0   // workgroups per CU of a many-message launch (0: no cap)
#endif
#ifndef WSG_FAN_MANY_WPC
#define WSG_FAN_MANY_WPC 46   // waves per CU per message of a many-message launch (0: as one message)
#endif
#ifndef WSG_FAN_MANY_WPB
#define WSG_FAN_MANY_WPB 0   // ... and waves per workgroup (0: as one message)
#endif
#ifndef WSG_FAN_KV
#define WSG_FAN_KV 2   // fan-out period path: key registers per lane (64 pass-window slots each)
#endif
#ifndef WSG_FAN_SC1
#define WSG_FAN_SC1 1   // fan-out period path: write-through (sc1) stores, 13.0 vs 14.3 us nontemporal at C4 (tools/tune_enc.py CFG=c4)
#endif

// Fan-out, flat kernel (frame sizes the period path does not take): the k frames are one byte stream of k * fsize bytes, cut into
// 16-byte chunks; every lane builds whole chunks (both frames' bytes where a
// frame boundary falls inside one), so every store is a full 16-B store and
// no cache line is written in parts by two waves.  The frame of a chunk is
// p / fsize (a double-precision reciprocal, corrected by one).
constexpr int FU = FAN_UNITS;

__device__ __forceinline__ uint32_t fan_byte(const uint8_t* __restrict__ payload, const uint32_t* __restrict__ keys,
                                             uint8_t opcode, bool mask, const SendGeom& g, uint64_t fsize, uint64_t i,
                                             uint64_t r)
{
    const uint32_t key = keys[i];
    if (r < g.hdr)
        return header_byte(opcode, mask, g.body, key, uint32_t(r));
    const uint64_t k = r - g.hdr;
    if (k < g.prefix)
        return key_byte(key, k);   // status 0: both prefix bytes are 0
    return uint32_t(payload[k - g.prefix]) ^ key_byte(key, k);
}

// Frames of one fan-out differ only in their key: the header + status bytes
// (data0 <= 16 of them) are a constant vector plus the key bytes.
struct FanGeom {
    SendGeom g;
    uint32_t data0;   // frame offset of the first payload byte (<= 16)
    uint32_t kpos;    // frame offset of the mask key (2 + ext)
    bool mask;
    v4u hp0;          // header with the key bytes left 0; status bytes 0
};

__device__ __forceinline__ FanGeom fan_geom(uint8_t opcode, bool mask, uint64_t len)
{
    FanGeom f;
    f.g = send_geom(opcode, mask, len, 0);
    f.data0 = f.g.hdr + f.g.prefix;
    f.kpos = f.g.hdr - (mask ? 4u : 0u);
    f.mask = mask;
    f.hp0 = v4u{0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < f.kpos; ++r)
        put_byte(f.hp0, r, header_byte(opcode, mask, f.g.body, 0, r));
    return f;
}

// Bytes [o, o + 16) of the frame with key `key` (bytes past the frame are 0).
__device__ __forceinline__ v4u fan_frame_bytes(const uint8_t* __restrict__ payload, uint64_t len, const FanGeom& f,
                                               uint64_t fsize, uint32_t key, uint64_t o)
{
    v4u hp = f.hp0;
    if (f.mask)
        hp |= shl_bytes(v4u{key, 0, 0, 0}, f.kpos);
    if (f.g.prefix)
        hp |= shl_bytes(v4u{key & 0xFFFFu, 0, 0, 0}, f.g.hdr);   // status 0 ^ key
    v4u out = shr_bytes(hp, o);
    const uint64_t lo = o < f.data0 ? f.data0 - o : 0;               // chunk bytes [lo, hi) are payload
    const uint64_t hi = fsize - o < CHUNK ? fsize - o : CHUNK;
    if (lo < hi) {
        const v4u w = fan_window(payload, len, int64_t(o) - int64_t(f.data0));
        const v4u m = low_bytes(hi) & ~low_bytes(lo);
        out |= (w ^ key_rot(key, uint32_t(o - f.g.hdr))) & m;
    }
    return out;
}

// Grid = `main_blocks` streaming blocks, then the edge blocks.
//  * Streaming waves own 64 x FU consecutive chunks and write every chunk
//    that is all payload of one frame (the frame index comes from one scalar
//    division per pass when frames are >= 1 KiB, else a per-lane reciprocal).
//  * Edge lanes own one (frame f, header chunk h) item each and write the
//    chunk(s) that hold frame f's start / header / status bytes, built from
//    frame f - 1's tail and frame f's head.  A chunk is written by exactly
//    one side (identical bytes if two edge items meet on one chunk), so the
//    streaming waves never branch into the header code.
//  * Frames shorter than a chunk: the streaming waves do every chunk byte by
//    byte and there are no edge blocks.
__device__ __forceinline__ void fan_locate(uint64_t p, uint64_t fsize, double inv, uint64_t& i, uint64_t& r)
{
    i = uint64_t(double(p) * inv);
    int64_t rr = int64_t(p - i * fsize);
    if (rr < 0) {
        --i;
        rr += int64_t(fsize);
    } else if (uint64_t(rr) >= fsize) {
        ++i;
        rr -= int64_t(fsize);
    }
    r = uint64_t(rr);
}

__device__ __forceinline__ void fan_store(uint8_t* __restrict__ wire, uint64_t c, uint64_t chunks, uint64_t total,
                                          v4u w)
{
    if (c + 1 < chunks || (total & (CHUNK - 1)) == 0) {
        st16nt(wire + c * CHUNK, w);
    } else {
#pragma unroll 1
        for (uint32_t j = 0; j < (total & (CHUNK - 1)); ++j)
            wire[c * CHUNK + j] = uint8_t(lane_byte(w, j));
    }
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_fanout_flat(const uint8_t* __restrict__ payload, uint64_t len,
                                                       const uint32_t* __restrict__ keys, uint32_t k, uint8_t opcode,
                                                       uint32_t mask, uint64_t fsize, double inv, uint32_t main_blocks,
                                                       uint8_t* __restrict__ wire)
{
    const FanGeom f = fan_geom(opcode, mask != 0, len);
    const SendGeom& g = f.g;
    const uint64_t total = fsize * k;
    const uint64_t chunks = (total + CHUNK - 1) / CHUNK;
    const uint64_t data0 = f.data0;
    const uint32_t lane = threadIdx.x & 63;

    // edge blocks come first in the grid so that their longer per-lane work
    // overlaps the streaming instead of trailing it
    const uint32_t edge_blocks = gridDim.x - main_blocks;
    if (blockIdx.x < edge_blocks) {
        // edge items: 2 per frame start (the last "start" is the wire's end)
        const uint64_t item = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
        const uint64_t fr = item >> 1, h = item & 1;
        if (fr > k || (WSG_DIAG_FAN & 8))
            return;
        const uint64_t start = fr * fsize;
        const uint64_t c = start / CHUNK + h;
        if (c >= chunks || (h && (start & (CHUNK - 1)) + data0 <= CHUNK) || (fr == k && h))
            return;
        uint64_t i, r;
        fan_locate(c * CHUNK, fsize, inv, i, r);
        v4u w = fan_frame_bytes(payload, len, f, fsize, keys[i], r);
        const uint64_t split = fsize - r;
        if (split < CHUNK && i + 1 < k)
            w |= shl_bytes(fan_frame_bytes(payload, len, f, fsize, keys[i + 1], 0), split);
        fan_store(wire, c, chunks, total, w);
        return;
    }

    const uint64_t step = uint64_t(main_blocks) * (BLOCK / 64) * (64 * FU);
    const bool big = fsize >= uint64_t(64) * CHUNK;   // a 1 KiB pass row spans at most 2 frames
    const uint32_t mb = blockIdx.x - edge_blocks;
    for (uint64_t base = (uint64_t(mb) * (BLOCK / 64) + wave_id()) * (64 * FU); base < chunks; base += step) {
        if (fsize < CHUNK) {
            // several frames per chunk: byte by byte
#pragma unroll 1
            for (int u = 0; u < FU; ++u) {
                const uint64_t c = base + uint64_t(u) * 64 + lane;
                if (c >= chunks)
                    break;
                uint64_t i, r;
                fan_locate(c * CHUNK, fsize, inv, i, r);
                v4u e = {0, 0, 0, 0};
#pragma unroll 1
                for (uint32_t j = 0; j < CHUNK; ++j, ++r) {
                    while (r >= fsize) {
                        r -= fsize;
                        ++i;
                    }
                    if (i < k)
                        put_byte(e, j, fan_byte(payload, keys, opcode, mask != 0, g, fsize, i, r));
                }
                fan_store(wire, c, chunks, total, e);
            }
            continue;
        }
        v4u v[FU];
        bool fast[FU];
        uint64_t i0 = 0, r0 = 0;
        if (big) {
            // frame of the pass row's first chunk: one scalar division per row
            i0 = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t((base * CHUNK) / fsize)));
            r0 = base * CHUNK - i0 * fsize;
        }
#pragma unroll
        for (int u = 0; u < FU; ++u) {
            const uint64_t c = base + uint64_t(u) * 64 + lane;
            uint64_t i, r;
            if (big) {
                // row u starts at most (FU - 1) KiB + r0 past frame i0's start
                r = r0 + (uint64_t(u) * 64 + lane) * CHUNK;
                i = i0;
#pragma unroll
                for (int q = 0; q < FU + 1; ++q)
                    if (r >= fsize) {
                        r -= fsize;
                        ++i;
                    }
            } else {
                fan_locate(c * CHUNK, fsize, inv, i, r);
            }
            fast[u] = c < chunks && r >= data0 && r + CHUNK <= fsize;
            v[u] = v4u{0, 0, 0, 0};
            if (fast[u]) {
                const v4u d = (WSG_DIAG_FAN & 2) ? v4u{uint32_t(r), 1, 2, 3}
                                                 : fan_window(payload, len, int64_t(r) - int64_t(data0));
                v[u] = d ^ key_rot((WSG_DIAG_FAN & 1) ? uint32_t(i) : keys[i], uint32_t(r - g.hdr));
            }
        }
#pragma unroll
        for (int u = 0; u < FU; ++u)
            if (fast[u])
                st16nt(wire + (base + uint64_t(u) * 64 + lane) * CHUNK, v[u]);
    }
}

hipError_t launch_fanout(hipStream_t s, int grid, const uint8_t* payload, uint64_t len, const uint32_t* keys,
                         uint32_t k, uint8_t opcode, uint32_t mask, uint64_t fsize, uint8_t* wire)
{
    // edge blocks: two items per frame start (k + 1 starts); none for
    // frames shorter than a chunk (the streaming waves do those)
    const uint64_t edge_blocks = fsize >= CHUNK ? (2 * (uint64_t(k) + 1) + BLOCK - 1) / BLOCK : 0;
    k_fanout_flat<<<dim3(uint32_t(grid + edge_blocks)), BLOCK, 0, s>>>(
        payload, len, keys, k, opcode, mask, fsize, 1.0 / double(fsize), uint32_t(grid), wire);
    return hipGetLastError();
}

// ---- fan-out, period path ---------------------------------------------------
// The k frames of a fan-out are one template (header + status + payload) and
// differ only in the key XORed over fixed byte positions.  With the frame size
// F a multiple of 4, every P = 16 / gcd(F, 16) (<= 4) consecutive frames form a
// group of G = P * F / 16 whole chunks, so a chunk's bytes depend only on its
// position j within its group and on the keys of the (<= 2) frames it touches:
//     chunk = T[j] ^ (MA[j] & rot(key_a)) ^ (MB[j] & rot(key_b)).
// With W waves (one per 64-thread block: 4-wave blocks measured slower) and W * 64 a multiple of G, a lane's j
// is the same in every pass, so it builds T / MA / MB once (the only payload
// loads) and then only stores, pass after pass, its chunk of successive groups.
// The wave's keys for all its passes come in one vector load up front (lane
// q holds key P * (first group of pass q / 2P) + q % 2P) and are picked per
// pass with a lane shuffle.  Rows are 1 KiB-aligned, whole lines per wave.
//
// Many messages in one launch (wsg_fanout_encode_many, the ws_multicast tick):
// blockIdx.y picks message y of up to FAN_MSGS messages of one geometry
// (length, opcode), whose payload and output start come from the kernel
// arguments; the k frames of every message are written exactly as for one.

namespace {

// Template and key mask of frame bytes [o, o + 16) (o < fsize): t = the
// bytes with a zero key (header with the key bytes 0, close status 0, raw
// payload; 0 past the frame), m = the bytes the key is XORed into ([kpos,
// fsize): mask key, status, payload), so the frame with key K is
// t ^ (m & key_rot(K, o - hdr)).
__device__ __forceinline__ void fan_tm(const uint8_t* __restrict__ payload, uint64_t len, const FanGeom& f,
                                       uint64_t fsize, uint64_t o, v4u& t, v4u& m)
{
    const uint64_t hi = fsize - o < CHUNK ? fsize - o : CHUNK;
    const uint64_t kl = o < f.kpos ? f.kpos - o : 0;
    const uint64_t lo = o < f.data0 ? f.data0 - o : 0;   // chunk bytes [lo, hi) are payload
    m = low_bytes(hi) & ~low_bytes(kl);
    t = shr_bytes(f.hp0, o);
    if (lo < hi)
        t |= fan_window(payload, len, int64_t(o) - int64_t(f.data0)) & (low_bytes(hi) & ~low_bytes(lo));
}

} // namespace

template <int P>
__global__ __launch_bounds__(1024) void k_fanout_period(const uint8_t* __restrict__ payload0, uint64_t len,
                                                      const uint32_t* __restrict__ keys, uint32_t k, uint8_t opcode,
                                                      uint32_t mask, uint64_t fsize, uint32_t G, uint32_t dm,
                                                      uint8_t* __restrict__ wire0, const FanMsgs msgs, v4u hp0,
                                                      uint32_t nwaves, uint32_t wpb)
{
    constexpr int KW = 2 * P;   // keys per pass: the row spans <= 2 groups (G >= 64)
    if (WSG_DIAG_FAN & 256)     // diagnostic: the launch of the grid alone
        return;
    const uint64_t src_off = msgs.src[blockIdx.y], dst_off = msgs.dst[blockIdx.y];
    // every kernel argument in SGPRs before anything else: left to the
    // compiler, the argument loads came in five dependent rounds (each
    // waiting on the last), a visible share of a 9 us kernel; this empty
    // asm consumes them all, so they are issued together and waited once
    asm volatile("" ::"s"(payload0), "s"(len), "s"(keys), "s"(k), "s"(fsize), "s"(G), "s"(dm), "s"(wire0),
                     "s"(nwaves), "s"(wpb), "s"(src_off), "s"(dst_off), "s"(uint32_t(opcode)), "s"(mask));
    const uint8_t* __restrict__ payload = payload0 + src_off;
    uint8_t* __restrict__ wire = wire0 + dst_off;
    FanGeom f;   // fan_geom() with the header bytes from the host (hp0)
    f.g = send_geom(opcode, mask != 0, len, 0);
    f.data0 = f.g.hdr + f.g.prefix;
    f.kpos = f.g.hdr - (mask ? 4u : 0u);
    f.mask = mask != 0;
    f.hp0 = hp0;
    const uint64_t total = fsize * k;
    const uint64_t chunks = (total + CHUNK - 1) / CHUNK;
    const uint32_t lane = threadIdx.x & 63;
    // one wave per block, W = nwaves of them (a kernel argument, not
    // gridDim: the dispatch packet is one more memory read before the first
    // store); rows are wave-uniform, so the write-through stores' buffer
    // resource sits in SGPRs (else every store becomes a waterfall loop)
    const uint32_t wid = blockIdx.x * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave of W
    if (wid >= nwaves)   // the last workgroup's spare waves
        return;
    const uint64_t row0 = uint64_t(wid) * 64;
    const uint64_t rstep = uint64_t(nwaves) * 64;   // W rows: a multiple of G (dm groups)
    const uint64_t m0 = uint32_t(row0) / G;              // first group of pass 0 (host: W < 2^22, row0 < 2^28)
    const uint32_t jw = uint32_t(row0 - m0 * G);         // group position of lane 0
    const uint32_t dl = (jw + lane) >= G ? 1u : 0u;      // lane's group: m0 + dl (+ it * dm)
    const uint32_t j = jw + lane - dl * G;

    // keys of every pass: slot it * KW + q -> key P * (m0 + it * dm) + q
    // (host: passes * KW <= 64 * WSG_FAN_KV).  Issued before the template's
    // payload loads, so the two arrive together: the kernel is short (41 MB
    // at C4), and a second dependent memory round trip before the first
    // store was a visible share of it
    uint32_t kv[WSG_FAN_KV];
#pragma unroll
    for (int h = 0; h < WSG_FAN_KV; ++h) {
        const uint32_t s = uint32_t(h) * 64 + lane;
        const uint64_t it = s / KW;
        const uint64_t idx = uint64_t(P) * (m0 + it * dm) + (s % KW);
        kv[h] = (WSG_DIAG_FAN & 32) ? uint32_t(idx) : (row0 + it * rstep < chunks && idx < k) ? keys[idx] : 0u;
    }

    // template of chunk j: its frame-a bytes, and the next frame's from byte
    // `split` on (the first 16 bytes of a frame: the same for every lane)
    const uint64_t o = uint64_t(j) * CHUNK;              // < P * fsize
    uint32_t qa = 0;                                     // frame of the group holding byte o
#pragma unroll
    for (int q = 1; q < P; ++q)
        qa += o >= uint64_t(q) * fsize ? 1u : 0u;
    const uint64_t r = o - uint64_t(qa) * fsize;
    v4u t, ma, mb = {0, 0, 0, 0};
    // a frame's first 16 bytes (the same for every lane), built by every
    // lane so that its payload loads go out with the chunk's own instead of
    // in a second round behind them; used where a frame starts in the chunk
    const uint64_t split = fsize - r;                    // the next frame starts at chunk byte `split`
    // (both windows issued together branch-free instead: +0.5 us per C4,
    // every lane then loads two more blocks; round 3)
    fan_tm(payload, len, f, fsize, r, t, ma);
    if (split < CHUNK) {
        v4u t0, m0v;
        fan_tm(payload, len, f, fsize, 0, t0, m0v);
        t |= shl_bytes(t0, split);
        mb = shl_bytes(m0v, split);
    }
    if (WSG_DIAG_FAN & 16) {
        t = v4u{j, 1, 2, 3};
        ma = v4u{~0u, ~0u, ~0u, ~0u};
    }
    const uint32_t pa = uint32_t(r - f.g.hdr), pb = uint32_t(0u - uint32_t(split) - f.g.hdr);
    const uint32_t ia = P * dl + qa;                     // key slots of this pass's window

    // Pass loop, kept lean (it is most of the kernel's instructions): running
    // row / pointer / shuffle-address registers instead of per-pass products,
    // rotations as one v_alignbit each, and a wave-uniform test for whole
    // rows, so a pass is ~2 shuffles, ~12 VALU and one 1 KiB store.
    const uint32_t sa = 8u * (pa & 3u), sbr = 8u * (pb & 3u);
    // rows below this are whole: 64 chunks, each all 16 bytes inside the
    // output (from whole chunks only: when the job's last chunk is partial
    // and ends a row, that row takes the byte-exact store below — counted
    // from `chunks`, its whole-chunk store wrote up to 15 bytes past the
    // last frame; profiles/r6/fan_gap_seed123.log)
    const uint64_t full_rows_end = (total / CHUNK) & ~uint64_t(63);
    // this wave's passes (rows row0 + it * rstep below chunks), the first
    // n_full of them whole rows: 32-bit scalar loop counters instead of
    // 64-bit row compares in the loop
    const uint32_t n_pass = row0 < chunks ? uint32_t((chunks - row0 + rstep - 1) / rstep) : 0u;
    const uint32_t n_full = row0 < full_rows_end ? uint32_t((full_rows_end - row0 + rstep - 1) / rstep) : 0u;
    const uint64_t wstep = rstep * CHUNK;
    const uint32_t addr = ia * 4;                           // shuffle address of key slot ia of pass 0
    if (WSG_DIAG_FAN & 128) {   // diagnostic: the prologue alone (its results kept live)
        const v4u w = t ^ ma ^ mb ^ v4u{kv[0], kv[WSG_FAN_KV - 1], addr, 0};
        if ((w[0] & w[1] & w[2] & w[3]) == 0xA5C3E1F7u && row0 + lane < chunks)
            st16nt(wire + (row0 + lane) * CHUNK, w);
        return;
    }
    // The keys of pass `it` for this lane: frame a's (slot ia) and, where a
    // frame starts inside the lane's chunk, frame b's (slot ia + 1).
    auto pass_keys = [&](uint32_t it, uint32_t& ka, uint32_t& kb, bool want_b) {
        const uint32_t slot = it * KW;                      // wave-uniform; KW divides 64
        uint32_t kreg = kv[0];
#pragma unroll
        for (int h = 1; h < WSG_FAN_KV; ++h)
            kreg = (slot >> 6) == uint32_t(h) ? kv[h] : kreg;
        const uint32_t sb = (slot & 63) * 4;
        ka = __builtin_amdgcn_ds_bpermute(int(addr + sb), int(kreg));
        kb = want_b ? __builtin_amdgcn_ds_bpermute(int(addr + sb + 4), int(kreg)) : 0u;
    };
    // The pass loop, in two forms: a frame starts inside a chunk at only
    // ~P positions of a group's G, so most waves hold no such lane (mb = 0
    // in every lane, fixed for all passes) and skip frame b's key and
    // masking; the loop is VALU-bound once the shuffles are off its chain.
    auto passes = [&](auto has_b) {
        constexpr bool B = decltype(has_b)::value;
        // a pass's keys are shuffled one pass ahead (in the pass itself:
        // C4 8.40 vs 8.32 us; v_readlane + per-lane selects 8.6, round 3)
        uint32_t ka_n = 0, kb_n = 0;
        pass_keys(0, ka_n, kb_n, B);
        auto word = [&](uint32_t it) {
            // this pass's keys were shuffled during the previous pass; the
            // next pass's go out now, ahead of this pass's store
            const uint32_t ka = ka_n, kb = kb_n;
            pass_keys(it + 1, ka_n, kb_n, B);   // (past the last pass: slots of kv, unused)
            const uint32_t ra = __builtin_amdgcn_alignbit(ka, ka, sa);
            v4u w = t ^ (ma & v4u{ra, ra, ra, ra});
            if constexpr (B) {
                const uint32_t rb = __builtin_amdgcn_alignbit(kb, kb, sbr);
                w ^= mb & v4u{rb, rb, rb, rb};
            }
            return w;
        };
        uint8_t* wrow = wire + row0 * CHUNK;
#pragma unroll FAN_UNROLL
        for (uint32_t it = 0; it < n_full; ++it) {
            const v4u w = word(it);
            if ((WSG_DIAG_FAN & 64) && (w[0] & w[1] & w[2] & w[3]) != 0xA5C3E1F7u) {
                // diagnostic: the computation without its stores
            } else if (WSG_FAN_SC1) {
                const OutTile ot(wrow, 64 * CHUNK, true);   // write-through (resource at the row)
                ot.put(lane * CHUNK, w);
            } else {
                st16nt(wrow + lane * CHUNK, w);
            }
            wrow += wstep;
        }
        if (n_pass > n_full) {   // the last, partial row (the job's final row only)
            const uint64_t row = row0 + uint64_t(n_full) * rstep;
            const v4u w = word(n_full);
            if (row + lane < chunks)
                fan_store(wire, row + lane, chunks, total, w);
        }
    };
    const bool any_b = __ballot((mb[0] | mb[1] | mb[2] | mb[3]) != 0u) != 0;   // wave-uniform
    if (any_b)
        passes(std::true_type{});
    else
        passes(std::false_type{});
}

// Period path (k_fanout_period) when the frame size allows it; returns false
// to leave the batch to k_fanout_flat.  Wave count W = Q * s with W * 64 a
// multiple of G (Q = G / gcd(G, 64)), about `waves` of them, and few enough
// passes per wave that one key load covers them (passes * 2P <= 64 * WSG_FAN_KV).
bool launch_fanout_period(hipStream_t s, int cus, int waves_per_cu, int wpb, const uint8_t* payload, uint64_t len,
                          const uint32_t* keys, uint32_t k, uint8_t opcode, uint32_t mask, uint64_t fsize,
                          uint8_t* wire, const FanMsgs& msgs, uint32_t nmsgs, hipError_t* err)
{
    if (nmsgs == 0 || nmsgs > uint32_t(FAN_MSGS))
        return false;
    if (!WSG_FAN_PERIOD || fsize % 4 != 0)
        return false;
    uint64_t g16 = 16;
    while (fsize % g16)
        g16 >>= 1;
    const uint32_t P = uint32_t(16 / g16);               // 1, 2 or 4
    const uint64_t G = uint64_t(P) * fsize / CHUNK;
    if (G < 64 || G > (1u << 20))
        return false;
    uint64_t g64 = 64;
    while (G % g64)
        g64 >>= 1;
    const uint64_t Q = G / g64;
    const uint64_t chunks = (fsize * k + CHUNK - 1) / CHUNK;
    const uint64_t max_passes = 64 * WSG_FAN_KV / (2 * P);
    if (Q * 64 > chunks * 2)   // even the fewest waves would mostly idle: leave it to the flat kernel
        return false;
    const uint64_t rows = (chunks + 63) / 64;
    if (WSG_FAN_MANY_WPC && nmsgs > 1)
        waves_per_cu = WSG_FAN_MANY_WPC;
    if (WSG_FAN_MANY_WPB && nmsgs > 1)
        wpb = WSG_FAN_MANY_WPB;
    uint64_t mult = std::max<uint64_t>(1, (uint64_t(cus) * waves_per_cu + Q / 2) / Q);
    mult = std::min(mult, (rows + Q - 1) / Q);                                                 // no idle waves
    mult = std::max(mult, (chunks + Q * 64 * max_passes - 1) / (Q * 64 * max_passes));   // every pass's keys in one load per lane
    const uint64_t W = Q * mult;
    if (W > (1u << 22))
        return false;
    const uint32_t dm = uint32_t(W * 64 / G);
    // workgroups of wpb waves (the last one's spare waves return at once):
    // dispatching one-wave workgroups was most of a C4 launch
    if (wpb < 1 || wpb > 16)
        wpb = 1;
    const uint32_t blocks = uint32_t((W + uint64_t(wpb) - 1) / uint64_t(wpb));
    // header bytes before the key (<= 10), the same in every frame
    const SendGeom sg = send_geom(opcode, mask != 0, len, 0);
    const uint32_t kpos = sg.hdr - (mask ? 4u : 0u);
    uint32_t hw[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < kpos; ++r)
        hw[r / 4] |= uint32_t(header_byte(opcode, mask != 0, sg.body, 0, r)) << (8 * (r % 4));
    const v4u hp0 = v4u{hw[0], hw[1], hw[2], hw[3]};
    // (WSG_FAN_CAP: LDS reserved per workgroup only to bound the workgroups
    // resident per CU; the kernel uses none)
    // (many messages only: one message's waves are all resident anyway)
    const uint32_t lds = WSG_FAN_CAP && nmsgs > 1 ? uint32_t((160u << 10) / WSG_FAN_CAP) & ~255u : 0u;
    switch (P) {
    case 1:
        k_fanout_period<1><<<dim3(blocks, nmsgs), 64 * uint32_t(wpb), lds, s>>>(payload, len, keys, k, opcode, mask, fsize,
                                                                             uint32_t(G), dm, wire, msgs, hp0, uint32_t(W),
                                                                             uint32_t(wpb));
        break;
    case 2:
        k_fanout_period<2><<<dim3(blocks, nmsgs), 64 * uint32_t(wpb), lds, s>>>(payload, len, keys, k, opcode, mask, fsize,
                                                                             uint32_t(G), dm, wire, msgs, hp0, uint32_t(W),
                                                                             uint32_t(wpb));
        break;
    default:
        k_fanout_period<4><<<dim3(blocks, nmsgs), 64 * uint32_t(wpb), lds, s>>>(payload, len, keys, k, opcode, mask, fsize,
                                                                             uint32_t(G), dm, wire, msgs, hp0, uint32_t(W),
                                                                             uint32_t(wpb));
        break;
    }
    *err = hipGetLastError();
    return true;
}

} // namespace wsg
