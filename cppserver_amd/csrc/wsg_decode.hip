// wsg_decode.hip — batched WebSocket frame decode (header unpack + payload
// unmask) in one launch on gfx950 (CDNA4): k_decode and launch_decode, the
// receive side of CppServer's WebSocket codec (reference
// source/server/ws/ws.cpp:320-406).
//
// Layout in HBM: wire (concatenated frames) -> out (same
// geometry, payloads unmasked where they sit); per-frame wsg_recv_info.
// Work unit: a 16 KiB tile of the OUTPUT byte range = 256 lanes x 16 B x 4.
// Every output byte is written exactly once by an aligned 16-byte
// nontemporal store (output is streamed, never re-read by the kernel).
//
// Each tile locates its frames itself with scalar loads and takes one of
// three block-uniform paths:
//   stream   - the tile lies inside one payload: 16-B load, XOR with the
//              tile-rotated key, 16-B store;
//   boundary - the tile touches <= MAXF frames: their payload segments are
//              held in scalar registers; a chunk inside a segment XORs with
//              its key word, the few chunks a segment edge cuts build masks;
//   staged   - more frames (small frames): segments staged in LDS, 256
//              frames per round.
// No MFMA: XOR is not a contraction; the bound is HBM bandwidth.
// The stages around a decoded batch are in wsg_messages.hip, wsg_frames.hip
// and wsg_utf8.hip; the host lane (wsg_lane_device.hip) decodes by the same
// rules (frame_parse_b, wsg_device.h).
#include "wsg_device.h"

namespace wsg {

namespace {

typedef uint64_t v4u64 __attribute__((ext_vector_type(4)));   // MAXF-wide frame fields

constexpr int MAXF = 4;   // frames a tile may touch and still take the boundary path

#ifndef WSG_DIAG
#define WSG_DIAG 0   // 5: timing-only diagnostic build of k_decode (every tile streams; tools/)
#endif
#ifndef WSG_DIAG_NOINFO
#define WSG_DIAG_NOINFO 0   // timing-only: k_decode without its per-frame info slice (tools/)
#endif
#ifndef WSG_DEC_WAVES
#define WSG_DEC_WAVES 1   // k_decode minimum waves/SIMD (register cap); 6 and 8 spill and run slower
#endif
#ifndef WSG_DEC_RELOAD
#define WSG_DEC_RELOAD 1   // k_decode staged tiles re-read their bytes instead of holding them in registers
#endif

#ifndef WSG_STAGE_FPL
#define WSG_STAGE_FPL 2
#endif
constexpr int SPL = WSG_STAGE_FPL;   // staged frames per lane per round
constexpr int LDSF = BLOCK * SPL;    // frames per staged round (one round for tiles of 32-byte frames)

__device__ __forceinline__ uint64_t lane_off(int u) { return (uint64_t(u) * BLOCK + threadIdx.x) * CHUNK; }

} // namespace

// ===========================================================================
// Decode in one launch: k_decode
// ===========================================================================
//
// Every tile finds its own frames.  The frame-start table is read-only and
// sorted, so the tile's first frame is located with uniform (scalar) loads:
// an interpolation guess, exact for equal-size frames, else a 16-ary search;
// the headers of the (at most MAXF) frames the tile touches are parsed from
// scalar loads of the wire.  Scalar loads do not queue behind the tile's
// vector data loads (those return in issue order), so this metadata chain
// overlaps the data's HBM latency.  The per-frame outputs (wsg_recv_info,
// error latch) come from a lane-per-frame slice of the same launch.  One
// launch instead of parse + unmask removes a kernel boundary: ~5 us per C2
// batch (tools/tune.py, a build that skipped the parse launch).
//
// Tile paths (block-uniform): stream (inside one payload), boundary (<= MAXF
// frames, records in scalar registers), staged (more frames: records staged
// in LDS, LDSF frames per round).

namespace {

__device__ __forceinline__ uint64_t fs_at(const uint64_t* __restrict__ fs, uint32_t n, int64_t i)
{
    return fs[min<int64_t>(i, int64_t(n) - 1)];   // clamped: the load never depends on a compare
}

// Last index i < b with fs[i] <= p, or a - 1, given fs[a - 1] <= p < fs[b]
// (fs[-1] = -inf, fs[n] = +inf): 8 independent probes per round (one round
// of scalar loads when a/b are uniform); ends for any table.
__device__ __forceinline__ int64_t search8(const uint64_t* __restrict__ fs, uint32_t a, uint32_t b, uint64_t p)
{
    while (a < b) {
        const uint32_t step = (b - a + 8) / 9;   // probes a - 1 + step * k, k = 1..8 (< b)
        uint64_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = fs[min(a - 1 + step * (k + 1), b - 1)];
        uint32_t na = a, nb = b;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t ix = min(a - 1 + step * (k + 1), b - 1);
            if (ix >= na && ix < nb) {
                if (v[k] <= p)
                    na = ix + 1;
                else
                    nb = ix;
            }
        }
        a = na;
        b = nb;
    }
    return int64_t(a) - 1;
}

// The frames a tile touches: first = max(f0, 0), where f0 is the last frame
// starting at or before the tile's first byte (-1: none); st[k] = fs[first+k]
// (~0 past the table).
struct TileLoc {
    int64_t f0;
    uint32_t first;
    uint64_t st[MAXF + 1];
};

// The tile's first-frame guess (exact for equal-size frames).
__device__ __forceinline__ uint64_t tile_guess(uint32_t n, double frames_per_byte, uint64_t base)
{
    return uni(min(uint64_t(double(base) * frames_per_byte), uint64_t(n - 1)));
}

// Lane k's entry of the coarse probe around the guess g: fs[g + (k - 32) S].
__device__ __forceinline__ uint32_t probe_index(uint64_t g, uint32_t stride, uint32_t n, int k)
{
    const int64_t i = int64_t(g) + int64_t(k - 32) * int64_t(stride);
    return uint32_t(max<int64_t>(0, min<int64_t>(i, int64_t(n) - 1)));
}

// Locate the tile's frames.  `probe` is this lane's coarse-probe entry,
// loaded before the tile's data (so it is back first).  Equal-size frames
// hit the guess (one round of scalar loads); otherwise the probe brackets
// the answer to `stride` frames (a miss outside +-32 strides searches the
// rest of the table), and search8 finishes it.
__device__ __forceinline__ void locate(const uint64_t* __restrict__ fs, uint32_t n, uint64_t g, uint32_t stride,
                                       uint64_t probe, uint64_t base, TileLoc& L)
{
    uint64_t w[MAXF + 2];
#pragma unroll
    for (int k = 0; k < MAXF + 2; ++k) {
        const uint64_t x = fs_at(fs, n, int64_t(g) + k);
        w[k] = (g + k < n) ? x : ~uint64_t(0);
    }
    if (w[0] <= base && base < w[1]) {   // the guess (equal-size frames)
        L.f0 = int64_t(g);
        L.first = uint32_t(g);
#pragma unroll
        for (int k = 0; k <= MAXF; ++k)
            L.st[k] = w[k];
        return;
    }
    // candidates [a, b) for the last start <= base, fs[a - 1] <= base < fs[b];
    // the probe is consulted only here, so a hit of the guess never waits for it
    const uint64_t below = __ballot(probe <= base);   // a prefix of the lanes for a sorted table
    const int m = __builtin_popcountll(below);
    uint32_t a = m > 0 ? probe_index(g, stride, n, m - 1) + 1 : 0;
    uint32_t b = m < 64 ? probe_index(g, stride, n, m) : n;
    if (m == 0 && probe_index(g, stride, n, 0) == 0)
        b = 0;   // even fs[0] is past base: no frame starts at or before it
    L.f0 = search8(fs, a, b, base);
    L.first = uint32_t(L.f0 < 0 ? 0 : L.f0);
#pragma unroll
    for (int k = 0; k <= MAXF; ++k) {
        const uint64_t x = fs_at(fs, n, int64_t(L.first) + k);
        L.st[k] = (uint64_t(L.first) + k < n) ? x : ~uint64_t(0);
    }
}

// A frame's payload as seen from one tile: bytes [lo, hi) of the tile
// (tile-relative, clamped to the tile; for the frames of a tile in order,
// lo and hi are non-decreasing) XOR with kr, the frame's key rotated
// to the tile's phase — chunk offsets are multiples of 16, so one rotation
// serves every chunk of the tile (ws.cpp:403: byte i uses key[i % 4]).
struct Seg {
    uint32_t lo, hi, kr;
};

__device__ __forceinline__ Seg tile_seg(uint64_t po, uint64_t pe, uint32_t key, uint64_t base, uint32_t span)
{
    Seg s;
    s.lo = po <= base ? 0u : uint32_t(min<uint64_t>(po - base, span));
    s.hi = pe <= base ? 0u : uint32_t(min<uint64_t>(pe - base, span));
    if (s.hi < s.lo)
        s.hi = s.lo;   // empty stays at its place: segment ends stay sorted
    s.kr = key_rot(key, uint32_t(base - po));   // (base - po) mod 4, also when po > base
    return s;
}

// The XOR word of segment s for the chunk at tile offset o (zero outside s).
__device__ __forceinline__ v4u seg_xor(uint32_t o, const Seg& s)
{
    if (s.hi <= o || s.lo >= o + CHUNK)
        return v4u{0, 0, 0, 0};
    const int a = s.lo > o ? int(s.lo - o) : 0;
    const int b = s.hi < o + CHUNK ? int(s.hi - o) : int(CHUNK);
    v4u m;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        m[d] = s.kr & low_bytes(b - 4 * d) & ~low_bytes(a - 4 * d);
    return m;
}

// A tile's inputs, issued before its metadata chain: the coarse probe of
// the frame table (vector load, first: loads return in issue order) and the
// tile's data.
struct TileIn {
    uint64_t base, g, probe;
    v4u v[UNROLL];
};

__device__ __forceinline__ void load_tile(TileIn& T, const uint8_t* __restrict__ wire, uint64_t wire_len,
                                          const uint64_t* __restrict__ fs, uint32_t n, double frames_per_byte,
                                          uint32_t stride, uint64_t base)
{
    T.base = base;
    T.g = tile_guess(n, frames_per_byte, base);
#if WSG_DIAG == 7   // timing-only: no coarse probe (right only where the guess is exact: equal-size frames)
    T.probe = 0;
#else
    T.probe = fs[probe_index(T.g, stride, n, int(threadIdx.x & 63))];
#endif
    __builtin_amdgcn_sched_barrier(0);
    // the tile's data does not depend on frame metadata: issue it next,
    // unconditionally, so that the metadata chain waits for the probe alone
    // (vmcnt(UNROLL)); loads behind a branch made the compiler wait vmcnt(0)
    // there, i.e. start the chain only once the whole tile had arrived.  The
    // wire's last, partial tile takes the staged path, which reads its bytes
    // itself: its loads here are clamped to the 16-B block holding the last
    // wire byte (readable by contract) and their values are not used.
    const uint64_t last_blk = (wire_len - 1) & ~uint64_t(CHUNK - 1);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        T.v[u] = ld16nt(wire + min(base + lane_off(u), last_blk));
}

// The tile's frames located, their segments XORed into its bytes, stored.
__device__ __forceinline__ void process_tile(const TileIn& T, const uint8_t* __restrict__ wire, uint8_t* out,
                                             uint64_t wire_len, const uint64_t* __restrict__ fs, uint32_t n,
                                             uint32_t stride)
{
    const uint64_t base = T.base;
    const uint64_t tend = min(base + TILE, wire_len);
    const uint32_t span = uint32_t(tend - base);
    const bool full = span == TILE;
    const uint64_t g = T.g;
    const uint64_t probe = T.probe;
    const v4u* v = T.v;
    // Only a guess miss reads the probe.  Used on that path alone, the load
    // would be sunk into it, behind the data loads (vector loads return in
    // issue order: a ragged tile would wait for its data before searching),
    // so every path ends with keep_probe(): a test that is never true for a
    // batch the host launches (n > 0), after the tile's stores, where the
    // probe is long back.
    auto keep_probe = [&]() {
        if (n == 0 && probe == ~uint64_t(0))
            out[0] = 0;
    };
    TileLoc L;
    locate(fs, n, g, stride, probe, base, L);
    // frames touching the tile: a prefix of first, first + 1, ...
    int c = 0;
#pragma unroll
    for (int k = 0; k <= MAXF; ++k) {
        const bool touches = uint64_t(L.first) + k < n && (k == 0 ? L.f0 >= 0 || L.st[0] < tend : L.st[k] < tend);
        if (touches && c == k)
            c = k + 1;
    }

    if (WSG_DIAG == 5 || (full && c <= MAXF)) {
        // frames' payload segments in scalar registers (full tiles; the
        // wire's last, partial tile takes the staged path)
        Seg S[MAXF];
#pragma unroll
        for (int k = 0; k < MAXF; ++k) {
            S[k] = Seg{0, 0, 0};
            if (k < c) {
                wsg_recv_info r;
                const uint64_t lim = (uint64_t(L.first) + k + 1 < n) ? L.st[k + 1] : wire_len;
                frame_parse(wire, wire_len, L.st[k], lim, r);
                const Seg g = tile_seg(r.payload_off, r.payload_off + r.len, r.key, base, span);
                S[k] = Seg{uni(g.lo), uni(g.hi), uni(g.kr)};
            }
        }
#if WSG_DIAG == 5   // timing-only: every tile streams with its first frame's key (8-wave register budget)
        if (true) {
#else
        if (S[0].lo == 0 && S[0].hi == TILE) {
#endif
            // stream: the whole tile is payload of one frame
            const OutTile ot(out + base, uint32_t(TILE));
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                ot.put(uint32_t(lane_off(u)), v[u] ^ S[0].kr);
            keep_probe();
            return;
        }
        const OutTile ot(out + base, uint32_t(TILE));
        // boundary: per chunk, the key word of the segment holding it;
        // the few chunks a segment edge cuts build byte masks
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t o = uint32_t(lane_off(u));
            uint32_t kx = 0;
            bool cut = false;
#pragma unroll
            for (int k = 0; k < MAXF; ++k) {
                kx = (S[k].lo <= o && o + CHUNK <= S[k].hi) ? S[k].kr : kx;
                cut |= (S[k].lo > o && S[k].lo < o + CHUNK) || (S[k].hi > o && S[k].hi < o + CHUNK);
            }
            v4u x = v4u{kx, kx, kx, kx};
            if (cut) {
                x = seg_xor(o, S[0]);
#pragma unroll
                for (int k = 1; k < MAXF; ++k)
                    x |= seg_xor(o, S[k]);
            }
            ot.put(o, v[u] ^ x);
        }
        keep_probe();
        return;
    }

    // staged: payload segments in LDS, LDSF frames per round
    __shared__ uint32_t s_lo[LDSF], s_hi[LDSF], s_kr[LDSF];
    __shared__ uint32_t s_wcnt[BLOCK / 64];
    // stage the segments of frames r0, r0 + 1, ... that touch the tile;
    // more = frames past the stage touch it too (block-uniform)
    auto stage = [&](uint64_t r0, int& cnt, bool& more) {
        // slot q * BLOCK + lane holds frame r0 + q * BLOCK + lane
        uint64_t sj[SPL], lim[SPL];
        bool touch[SPL];
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const uint64_t fi = r0 + uint64_t(q) * BLOCK + threadIdx.x;
            sj[q] = ~uint64_t(0);
            lim[q] = wire_len;
            if (fi < n) {
                sj[q] = fs[fi];
                lim[q] = fi + 1 < n ? fs[fi + 1] : wire_len;
            }
            // frame `first` touches (c > MAXF); the others when they start in the tile
            touch[q] = fi < n && (fi == L.first || sj[q] < tend);
        }
        // block-wide counts from wave ballots through LDS (the
        // __syncthreads_count / _or builtins cost ~40 VGPRs here,
        // tools/regs.py: 91 vs 53 for the whole kernel)
        uint32_t wc = 0;
#pragma unroll
        for (int q = 0; q < SPL; ++q)
            wc += uint32_t(__builtin_popcountll(__ballot(touch[q])));
        const bool last_more = __ballot(threadIdx.x == BLOCK - 1 && touch[SPL - 1] &&
                                        r0 + uint64_t(LDSF) < n && lim[SPL - 1] < tend) != 0;
        __syncthreads();   // the previous readers are done with the stage and the counts
        if ((threadIdx.x & 63) == 0)
            s_wcnt[threadIdx.x >> 6] = wc | (last_more ? 0x80000000u : 0u);
        __syncthreads();
        cnt = 0;
        more = false;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            const uint32_t x = s_wcnt[w];
            cnt += int(x & 0x7FFFFFFFu);
            more = more || (x >> 31) != 0;
        }
#pragma unroll 1
        for (int q = 0; q < SPL; ++q) {
            const int slot = q * BLOCK + int(threadIdx.x);
            if (slot < cnt) {
                wsg_recv_info r;
                frame_parse(wire, wire_len, sj[q], lim[q], r);
                const Seg g = tile_seg(r.payload_off, r.payload_off + r.len, r.key, base, span);
                s_lo[slot] = g.lo;
                s_hi[slot] = g.hi;
                s_kr[slot] = g.kr;
            }
        }
        __syncthreads();
    };
    // XOR words of the staged segments for the chunk at tile offset o
    auto chunk_xor = [&](uint32_t o, int cnt) {
        int lo = 0, hi = cnt;   // first segment ending after o (segment ends are non-decreasing)
#pragma unroll 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_hi[mid] <= o)
                lo = mid + 1;
            else
                hi = mid;
        }
        v4u x = {0, 0, 0, 0};
#pragma unroll 1
        for (int j = lo; j < cnt && s_lo[j] < o + CHUNK; ++j)
            x |= seg_xor(o, Seg{s_lo[j], s_hi[j], s_kr[j]});
        return x;
    };
    // rounds of LDSF frames (one for every tile but those of the tiniest
    // frames): each round ORs its segments' XOR words into the thread's
    // own LDS slots, then one pass reads the tile's bytes again (L2 /
    // Infinity-Cache warm), XORs and stores.  Nothing is carried in
    // registers across the staging: this path would otherwise set the
    // kernel's register budget (95 VGPRs with the tile held in registers
    // and a per-round store, 5 waves/SIMD; tools/regs.py).
    __shared__ v4u s_acc[UNROLL][BLOCK];
#pragma unroll 1
    for (uint64_t r0 = L.first;; r0 += LDSF) {
        int cnt;
        bool more;
        stage(r0, cnt, more);
#pragma unroll 1
        for (int u = 0; u < UNROLL; ++u) {
            const v4u x = chunk_xor(uint32_t(lane_off(u)), cnt);
            s_acc[u][threadIdx.x] = (r0 == L.first) ? x : (s_acc[u][threadIdx.x] | x);
        }
        if (!more)
            break;
    }
    {
        const OutTile ot(out + base, uint32_t(TILE));
#pragma unroll 1
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t o = uint32_t(lane_off(u));
            if (o + CHUNK <= span) {
                ot.put(o, ld16(wire + base + o) ^ s_acc[u][threadIdx.x]);
            } else if (o < span) {
                // the chunk the wire's end cuts: bytes only, through the
                // thread's LDS slot (no register byte shuffles)
                uint8_t* b = reinterpret_cast<uint8_t*>(&s_acc[u][threadIdx.x]);
#pragma unroll 1
                for (uint32_t k = 0; k < span - o; ++k)
                    out[base + o + k] = uint8_t(wire[base + o + k] ^ b[k]);
            }
        }
    }
    keep_probe();
}

} // namespace

// Decode (ws.cpp:320-406 over a batch): out = wire with every payload XORed
// by its key; info[i] and the error latch per frame.
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WSG_DEC_WAVES))) void k_decode(const uint8_t* __restrict__ wire, uint8_t* out, uint64_t wire_len,
                                                  const uint64_t* __restrict__ fs, uint32_t n, double frames_per_byte,
                                                  uint32_t stride, wsg_recv_info* __restrict__ info,
                                                  unsigned long long* err, uint64_t num_tiles)
{
    // per-frame slice: header unpack + checks, one lane per frame (on the
    // grid's last blocks after their tiles instead: no faster, round 3)
    {
        const uint64_t fstride = uint64_t(gridDim.x) * BLOCK;
        for (uint64_t i0 = uint64_t(blockIdx.x) * BLOCK + (threadIdx.x & ~63u); i0 < n && !WSG_DIAG_NOINFO;
             i0 += fstride) {
            const uint64_t i = i0 + (threadIdx.x & 63u);
            if (i < n) {
                wsg_recv_info r;
                const int e = frame_parse(wire, wire_len, fs[i], i + 1 < n ? fs[i + 1] : wire_len, r);
                if (e != 0)
                    latch(err, i, e);
                store_info(info + i, r);
            }
        }
    }

#if WSG_DIAG == 6   // timing-only: the launch as a bare copy-with-XOR of the full tiles (no frame logic)
    for (uint64_t t = blockIdx.x; t < num_tiles; t += gridDim.x) {
        const uint64_t base = t * TILE;
        if (base + TILE > wire_len)
            break;
        v4u v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            v[u] = ld16nt(wire + base + lane_off(u));
#ifdef WSG_DIAG_ORD
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            st16nt(out + base + lane_off(u), v[u] ^ 0x9u);
    }
    return;
#endif
    // (two tiles per block with both tiles' loads up front: 0.0900 vs 0.0875
    // ms at C2, round 2, dropped)
    for (uint64_t t = blockIdx.x; t < num_tiles; t += gridDim.x) {
        TileIn a;
        load_tile(a, wire, wire_len, fs, n, frames_per_byte, stride, t * TILE);
        process_tile(a, wire, out, wire_len, fs, n, stride);
    }
}

hipError_t launch_decode(hipStream_t s, int grid, const uint8_t* wire, uint8_t* out, uint64_t wire_len,
                         const uint64_t* fs, uint32_t n, wsg_recv_info* info, unsigned long long* err)
{
    const uint64_t tiles = (wire_len + TILE - 1) / TILE;
    // frames per wire byte: the tile's first-frame guess (exact for equal-size frames)
    const double fpb = wire_len ? double(n) / double(wire_len) : 0.0;
    // coarse-probe stride: 64 probes span +-32 strides around the guess, a
    // power of two >= sqrt(n) / 32 frames (a random-walk deviation of frame
    // counts from the guess grows like sqrt(n): C3's 65536 ragged frames
    // deviate by ~100)
    uint32_t stride = 1;
    while (uint64_t(stride) * stride * 1024 < n)
        stride <<= 1;
    k_decode<<<grid, BLOCK, 0, s>>>(wire, out, wire_len, fs, n, fpb, stride, info, err, tiles);
    return hipGetLastError();
}

} // namespace wsg
