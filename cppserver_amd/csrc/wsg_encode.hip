// wsg_encode.hip — batched WebSocket frame encode (header pack + payload
// mask) on gfx950 (CDNA4), the send side of CppServer's WebSocket codec
// (reference source/server/ws/ws.cpp:212-318): payload arena +
// wsg_send_desc[] -> wire (frames back to back).
//   piece encode       - the scan kernels size the frames and cut them into
//                        pieces, k_encode_mask writes them, a wave per piece;
//   small-frame encode - k_encode_small, a block per group of consecutive
//                        frames, picked by the host when the average frame is
//                        small; its chunk builder (wsg_small_frame.h) is
//                        shared with the host lane.
// Every output byte is written exactly once, whole 16-byte chunks by aligned
// nontemporal stores.
#include "wsg_small_frame.h"

namespace wsg {

// ===========================================================================
// Encode: frame-aligned work pieces
// ===========================================================================
//
// A piece is at most PIECE = 4 KiB of ONE frame's wire bytes, cut at absolute
// 16-byte chunk boundaries: piece k of frame i covers
//     [max(off_i, A_i + k*PIECE), min(end_i, A_i + (k+1)*PIECE)),   A_i = off_i & ~127
// (line-aligned output rows).
// One wave encodes one piece, so the key, the key phase and the source shift
// are uniform over it: full data chunks stream (aligned 16-B loads,
// v_alignbyte_b32 funnel, XOR, 16-B nontemporal store).  Chunks holding
// header / close-status bytes, and the two edge chunks a frame shares with
// its neighbours, are built bytewise (edge chunks: each frame stores only
// its own bytes).  Piece counts are scanned together with frame sizes.

namespace {

#ifndef WSG_ENC_NT_SRC
#define WSG_ENC_NT_SRC 0   // encode payload loads: plain policy measured 1-5% faster than nontemporal
#endif
#ifndef WSG_ENC_NT_HI
#define WSG_ENC_NT_HI 1    // ... including the funnel's second block (the next lane's line)
#endif
#ifndef WSG_DIAG_ENC
#define WSG_DIAG_ENC 0   // timing-only encode diagnostics: 1 skip edge chunks, 2 no funnel
#endif
#ifndef WSG_ENC_SC1
#define WSG_ENC_SC1 0   // batch encode (piece kernel): write-through stores (A/B)
#endif

// map[t] = frame for t in [lo, hi) (encode: piece -> frame), for every lane's range, with the
// whole wave storing each range (one lane per frame would serialise a large
// frame's thousands of tiles on a single lane).
__device__ __forceinline__ void fill_tiles_wave(uint32_t* tile_first, uint64_t lo, uint64_t hi, uint32_t frame)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr uint64_t kShort = 16;   // ranges up to this many entries: the lane stores its own
    if (hi > lo && hi - lo <= kShort)
        for (uint64_t t = lo; t < hi; ++t)
            tile_first[t] = frame;
    uint64_t pending = __ballot(hi > lo + kShort);
    while (pending) {
        const int j = __builtin_ctzll(pending);
        pending &= pending - 1;
        const uint64_t a = lane_bcast(lo, j), b = lane_bcast(hi, j);
        const uint32_t fj = __builtin_amdgcn_readlane(frame, j);
        for (uint64_t t = a + lane; t < b; t += 64)
            tile_first[t] = fj;
    }
}

// edge_chunk built with 16-byte vector operations instead of a byte loop:
// the head shifted into place, the data window XORed with the rotated key
// under its byte mask; stored whole when every byte is this frame's, else
// by dwords (bytes only where a dword is shared with a neighbour).
__device__ __forceinline__ void edge_chunk2(const FrameRec& R, v4u head, uint64_t p, uint8_t* __restrict__ wire)
{
    if (p + CHUNK <= R.off)
        return;   // a chunk of the piece's line before the frame: a neighbour's
    v4u w = p >= R.off ? shr_bytes(head, p - R.off) : shl_bytes(head, R.off - p);
    const int64_t data_len = int64_t(R.end - R.data_w);
    const int64_t rel = int64_t(p) - int64_t(R.data_w);   // source offset of chunk byte 0
    if (rel < data_len && rel + int64_t(CHUNK) > 0) {
        const v4u d = fan_window(R.src, uint64_t(data_len), rel);
        const uint32_t kw = key_rot(R.key, uint32_t(p - R.pw));   // (mod 4 also when p < pw)
        const uint64_t lo = p < R.data_w ? R.data_w - p : 0;
        const uint64_t hi = R.end - p < CHUNK ? R.end - p : CHUNK;
        w |= (d ^ v4u{kw, kw, kw, kw}) & (low_bytes(hi) & ~low_bytes(lo));
    }
    const uint32_t o_lo = p < R.off ? uint32_t(R.off - p) : 0u;
    const uint32_t o_hi = R.end - p < CHUNK ? uint32_t(R.end - p) : uint32_t(CHUNK);
    if ((o_lo == 0 && o_hi == CHUNK) || (WSG_DIAG_ENC & 4)) {
        st16nt(wire + p, w);
        return;
    }
    uint32_t* w32 = reinterpret_cast<uint32_t*>(wire + p);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b0 = 4 * k, b1 = b0 + 4;
        if (b0 >= o_lo && b1 <= o_hi) {
            w32[k] = w[k];
        } else {
            for (uint32_t j = max(b0, o_lo); j < min(b1, o_hi); ++j)
                wire[p + j] = uint8_t(w[k] >> (8 * (j - b0)));
        }
    }
}

// One wave's piece k of frame R, in two phases so that a wave can keep two
// pieces' loads in flight before storing either (load(), then store()).
template <bool NT>
struct Piece {
    FrameRec R;
    uint64_t lo = 0, hi = 0;
    uint32_t s = 0;        // source misalignment, uniform over the piece
    uint32_t kw = 0;       // key rotated to the piece's phase (uniform)
    bool live = false;
    uint32_t dmask = 0;   // bit u: chunk u of this lane is all data (a bool array would land in LDS)
    v4u a[EU], b[EU];

    __device__ __forceinline__ void load(const FrameRec& rec, uint64_t k, bool exists)
    {
        R = rec;
        const uint32_t lane = threadIdx.x & 63;
        lo = (R.off & ~(PIECE_ALIGN - 1)) + k * PIECE;
        live = exists && lo < R.end;   // piece counts are an upper bound
        hi = min(lo + PIECE, R.end);
        // source of wire byte q: R.src + (q - R.data_w), as pointer
        // arithmetic on the payload argument (global_* loads; a uintptr_t
        // round trip made them flat loads, whose lgkmcnt share turned every
        // scalar-load wait of the descriptor pipeline into a data-load wait)
        s = (WSG_DIAG_ENC & 2) ? 0u
                                : uint32_t((reinterpret_cast<uintptr_t>(R.src) + (lo - R.data_w)) & 15u);
        kw = key_rot(R.key, uint32_t(lo - R.pw));
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            const bool d = live && p < hi && p >= R.data_w && p + CHUNK <= R.end;
            dmask |= uint32_t(d) << u;
            const uint8_t* a0 = R.src + (int64_t(p - R.data_w) - int64_t(s));
            a[u] = d ? (NT ? ld16nt(a0) : ld16(a0)) : v4u{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            const uint8_t* a0 = R.src + (int64_t(p - R.data_w) - int64_t(s));
            b[u] = ((dmask >> u) & 1u) && s ? ((NT && WSG_ENC_NT_HI) ? ld16nt(a0 + CHUNK) : ld16(a0 + CHUNK))
                                          : v4u{0, 0, 0, 0};
        }
    }

    __device__ __forceinline__ void store(uint8_t* __restrict__ wire) const
    {
        if (!live)
            return;
        const uint32_t lane = threadIdx.x & 63;
        const OutTile ot(wire + lo, uint32_t(PIECE), WSG_ENC_SC1 != 0);
        v4u head = {0, 0, 0, 0};
        if (lo < R.data_w)   // (wave-uniform) the piece holds header / status bytes
            head = frame_head(R);
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const uint64_t p = lo + (uint64_t(u) * 64 + lane) * CHUNK;
            if ((dmask >> u) & 1u) {
                ot.put(uint32_t(p - lo), (s ? funnel(a[u], b[u], s) : a[u]) ^ kw);
            } else if (p < hi && !(WSG_DIAG_ENC & 1)) {
                // header / status bytes, or a chunk shared with a neighbour
                // (built as a vector: the byte-at-a-time build it replaced
                // made C3's encode 0.730 ms against 0.701, round 4)
                edge_chunk2(R, head, p, wire);
            }
        }
    }
};

__device__ __forceinline__ uint64_t pieces_of(uint64_t frame_bytes)
{
    return (frame_bytes + PIECE_ALIGN - 1 + PIECE - 1) / PIECE;
}

} // namespace

// Per-block local exclusive scans of frame sizes and piece counts
// (SCAN_ITEMS frames per block).  Round k of a block reads frames
// k * BLOCK + t, so consecutive lanes read consecutive descriptors (a lane
// reading SCAN_PER_LANE adjacent descriptors touched 64 lines per load
// instruction); the rounds scan in frame order, carrying the running sums.
// PIECES = false (small-frame path): no piece counts.
template <bool PIECES>
__global__ __launch_bounds__(BLOCK) void k_encode_scan_local(const wsg_send_desc* __restrict__ desc, uint32_t n,
                                                             uint64_t* __restrict__ wire_off,
                                                             uint32_t* __restrict__ piece_start,
                                                             uint64_t* __restrict__ block_sums,
                                                             uint64_t* __restrict__ block_psums)
{
    const uint64_t first = uint64_t(blockIdx.x) * SCAN_ITEMS;
    uint64_t sz[SCAN_PER_LANE];
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k) {   // all descriptor loads first
        const uint64_t i = first + uint64_t(k) * BLOCK + threadIdx.x;
        sz[k] = 0;
        if (i < n) {
            const Desc d = load_desc(desc + i);
            const SendGeom g = send_geom(d.opcode, d.mask, d.len, d.status);
            sz[k] = g.hdr + g.body;
        }
    }
    uint64_t run = 0, run_p = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k) {
        const uint64_t i = first + uint64_t(k) * BLOCK + threadIdx.x;
        uint64_t tot, tot_p = 0;
        const uint64_t ex = block_scan_ex(sz[k], OpAdd{}, &tot);
        uint64_t ex_p = 0;
        if (PIECES)
            ex_p = block_scan_ex(sz[k] ? pieces_of(sz[k]) : 0, OpAdd{}, &tot_p);
        if (i < n) {
            wire_off[i] = run + ex;
            if (PIECES)
                piece_start[i] = uint32_t(run_p + ex_p);
        }
        run += tot;
        run_p += tot_p;
    }
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = run;
        if (PIECES)
            block_psums[blockIdx.x] = run_p;
    }
}

// Single block: exclusive scans of the block sums; wire_off[n] = total bytes,
// piece_start[n] = total pieces.
__global__ __launch_bounds__(BLOCK) void k_encode_scan_blocks(const uint64_t* __restrict__ block_sums,
                                                              const uint64_t* __restrict__ block_psums, uint32_t nb,
                                                              uint64_t* __restrict__ block_prefix,
                                                              uint64_t* __restrict__ block_pprefix,
                                                              uint64_t* __restrict__ wire_off,
                                                              uint32_t* __restrict__ piece_start, uint32_t n)
{
    const uint64_t carry = scan_partials(block_sums, block_prefix, nb, OpAdd{});
    const uint64_t carry_p = scan_partials(block_psums, block_pprefix, nb, OpAdd{});
    if (threadIdx.x == 0) {
        wire_off[n] = carry;
        piece_start[n] = uint32_t(carry_p);
    }
}

// Add block prefixes, build the piece -> frame map, check capacity.
__global__ __launch_bounds__(BLOCK) void k_encode_finalize(const wsg_send_desc* __restrict__ desc, uint32_t n,
                                                           uint64_t* __restrict__ wire_off,
                                                           uint32_t* __restrict__ piece_start,
                                                           const uint64_t* __restrict__ block_prefix,
                                                           const uint64_t* __restrict__ block_pprefix,
                                                           uint32_t* __restrict__ piece_frame, uint64_t pieces_cap,
                                                           uint64_t wire_cap, unsigned long long* err)
{
    if (blockIdx.x * BLOCK + (threadIdx.x & ~63u) >= n)
        return;   // whole wave past the last frame
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint64_t lo = 0, hi = 0;
    if (i < n) {
        const wsg_send_desc d = desc[i];
        const SendGeom g = send_geom(d.opcode, d.mask != 0, d.len, d.status);
        const uint64_t off = wire_off[i] + block_prefix[i / SCAN_ITEMS];
        const uint64_t ps = piece_start[i] + block_pprefix[i / SCAN_ITEMS];
        const uint64_t end = off + g.hdr + g.body;
        wire_off[i] = off;
        piece_start[i] = uint32_t(ps);
        if (end > wire_cap)
            latch(err, i, WSG_ENOMEM);
        piece_range(ps, ps + pieces_of(g.hdr + g.body), pieces_cap, lo, hi);
    }
    fill_tiles_wave(piece_frame, lo, hi, i);
}

__global__ __launch_bounds__(BLOCK) void k_encode_mask(const uint8_t* __restrict__ payload,
                                                       const wsg_send_desc* __restrict__ desc, uint32_t n,
                                                       const uint64_t* __restrict__ wire_off,
                                                       const uint32_t* __restrict__ piece_start,
                                                       const uint32_t* __restrict__ piece_frame,
                                                       uint8_t* __restrict__ wire, uint64_t wire_cap,
                                                       uint32_t q_begin, uint32_t q_end)
{
    const uint32_t waves = gridDim.x * (BLOCK / 64);
    uint32_t q = q_begin + blockIdx.x * (BLOCK / 64) + wave_id();
    if (wire_off[n] > wire_cap)
        return;   // capacity error latched by k_encode_finalize
    const uint32_t pieces = min(piece_start[n], q_end);   // this launch's pieces: [q_begin, min(all pieces, q_end))
    // Software pipeline over the wave's pieces: while piece q streams, the
    // descriptor of piece q + W (frame index already known) and the frame
    // index of piece q + 2W are in flight, so the dependent metadata loads
    // never sit between a piece's data loads and the previous piece's stores.
    struct Meta {
        Desc d;
        uint64_t off;
        uint32_t ps;
    };
    auto meta = [&](uint32_t i) { return Meta{load_desc(desc + i), wire_off[i], piece_start[i]}; };
    if (q >= pieces)
        return;
    Meta cur = meta(piece_frame[q]);
    uint32_t i_next = (q + waves < pieces) ? piece_frame[q + waves] : 0;
    for (;;) {
        Piece<WSG_ENC_NT_SRC != 0> pc;
        pc.load(make_rec(cur.off, payload + cur.d.src_off, cur.d.len, cur.d.key, cur.d.status, cur.d.opcode,
                         cur.d.mask),
                q - cur.ps, true);
        const uint32_t qn = q + waves;
        const bool more = qn < pieces;
        Meta nxt = cur;
        uint32_t i_after = 0;
        if (more) {
            nxt = meta(i_next);
            i_after = (qn + waves < pieces) ? piece_frame[qn + waves] : 0;
        }
        pc.store(wire);
        if (!more)
            break;
        cur = nxt;
        i_next = i_after;
        q = qn;
    }
}

hipError_t launch_encode_scan(hipStream_t s, const wsg_send_desc* desc, uint32_t n, uint64_t* wire_off,
                              uint32_t* piece_start, uint64_t* scan, uint32_t* piece_frame, uint64_t pieces_cap,
                              uint64_t wire_cap, unsigned long long* err)
{
    const uint32_t nb = uint32_t((n + SCAN_ITEMS - 1) / SCAN_ITEMS);
    uint64_t* sums = scan;
    uint64_t* psums = scan + nb;
    uint64_t* prefix = scan + 2 * uint64_t(nb);
    uint64_t* pprefix = scan + 3 * uint64_t(nb);
    k_encode_scan_local<true><<<nb, BLOCK, 0, s>>>(desc, n, wire_off, piece_start, sums, psums);
    k_encode_scan_blocks<<<1, BLOCK, 0, s>>>(sums, psums, nb, prefix, pprefix, wire_off, piece_start, n);
    k_encode_finalize<<<(n + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(desc, n, wire_off, piece_start, prefix, pprefix,
                                                                piece_frame, pieces_cap, wire_cap, err);
    return hipGetLastError();
}

hipError_t launch_encode_mask(hipStream_t s, int grid, const uint8_t* payload, const wsg_send_desc* desc, uint32_t n,
                              const uint64_t* wire_off, const uint32_t* piece_start, const uint32_t* piece_frame,
                              uint8_t* wire, uint64_t wire_cap, uint32_t q_begin, uint32_t q_end)
{
    k_encode_mask<<<grid, BLOCK, 0, s>>>(payload, desc, n, wire_off, piece_start, piece_frame, wire, wire_cap, q_begin,
                                         q_end);
    return hipGetLastError();
}

// ---- batch encode of small frames -----------------------------------------
// The piece kernel spends one wave pass per frame whatever its size, so a
// batch of frames a few dozen bytes long (the reference's 32-byte echo
// messages) leaves most lanes idle.  Here a block owns fpb <= SMALL_F
// consecutive frames (about SMALL_RANGE wire bytes at the batch's average
// frame size), i.e. one contiguous wire range, and its lanes own the 16-B chunks
// of that range.  A chunk is ORed together from the frames it overlaps: each
// frame's head (header + close-status bytes, <= 16, built once per frame into
// LDS) shifted into place, plus its masked payload window.  The chunks at the
// two ends of the range, shared with the neighbouring blocks, get byte stores
// of this block's bytes only.  Correct for any sizes; the host picks it when
// the average frame is small (SMALL_AVG).
static_assert(SMALL_F <= BLOCK && SCAN_ITEMS % SMALL_F == 0, "k_encode_small: one frame per lane, one scan block");

// Also finishes the offsets scan (k_encode_scan_blocks and
// k_encode_finalize for the piece path): wire_off holds the block-local
// offsets of k_encode_scan_local<false>, block_sums its nb block totals; a
// block's frames share one scan block (fpb divides SCAN_ITEMS), whose prefix
// the block sums from the L2-resident totals itself.
__global__ __launch_bounds__(BLOCK) void k_encode_small(const uint8_t* __restrict__ payload,
                                                        const wsg_send_desc* __restrict__ desc, uint32_t n,
                                                        uint32_t fpb, uint64_t* __restrict__ wire_off,
                                                        const uint64_t* __restrict__ block_sums, uint32_t nb,
                                                        uint8_t* __restrict__ wire, uint64_t wire_cap,
                                                        unsigned long long* err)
{
    __shared__ uint64_t s_off[SMALL_F + 1];
    __shared__ v4u s_head[SMALL_F];
    __shared__ SmallFrame s_fr[SMALL_F];
    const uint32_t f_lo = blockIdx.x * fpb;   // fpb <= SMALL_F (host)
    if (f_lo >= n)
        return;
    const uint32_t sb = f_lo / uint32_t(SCAN_ITEMS);
    const uint32_t cnt = min(n - f_lo, fpb);
    const uint32_t t = threadIdx.x;   // frame f_lo + t (cnt <= BLOCK)
    // every load first (scan-block totals, descriptor, local offset), so that
    // their round trips overlap
    constexpr int PB = 4;   // totals per lane in one go (1 Mi frames); more in the loop below
    uint64_t bs[PB];
#pragma unroll
    for (int u = 0; u < PB; ++u) {
        const uint32_t k = t + uint32_t(u) * BLOCK;
        bs[u] = k < nb ? block_sums[k] : 0;
    }
    Desc d{};
    uint64_t off_local = 0;
    if (t < cnt) {
        d = load_desc(desc + f_lo + t);
        off_local = wire_off[f_lo + t];
    }
    uint64_t sz = 0;
    if (t < cnt)
        sz = small_head(d, s_head[t], s_fr[t]);
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int u = 0; u < PB; ++u) {
        all += bs[u];
        before += t + uint32_t(u) * BLOCK < sb ? bs[u] : 0;
    }
    for (uint32_t k = t + PB * BLOCK; k < nb; k += BLOCK) {
        const uint64_t v = block_sums[k];
        all += v;
        before += k < sb ? v : 0;
    }
    uint64_t prefix, total;
    (void)block_scan_ex(before, OpAdd{}, &prefix);
    (void)block_scan_ex(all, OpAdd{}, &total);
    if (blockIdx.x == 0 && t == 0)
        wire_off[n] = total;
    const bool over = total > wire_cap;
    if (t < cnt) {
        const uint32_t i = f_lo + t;
        const uint64_t off = off_local + prefix;
        const uint64_t end = off + sz;
        wire_off[i] = off;
        s_off[t] = off;
        if (t + 1 == cnt)
            s_off[cnt] = end;   // not from wire_off[i + 1]: the next block may have finalized it already
        if (end > wire_cap)
            latch(err, i, WSG_ENOMEM);
    }
    __syncthreads();
    if (over)
        return;   // offsets are final and the error latched; no frame bytes
    small_chunks(payload, s_off, s_head, s_fr, cnt, wire, threadIdx.x, BLOCK);
}

hipError_t launch_encode_scan_small(hipStream_t s, const wsg_send_desc* desc, uint32_t n, uint64_t* wire_off,
                                    uint64_t* scan)
{
    const uint32_t nb = uint32_t((n + SCAN_ITEMS - 1) / SCAN_ITEMS);
    k_encode_scan_local<false><<<nb, BLOCK, 0, s>>>(desc, n, wire_off, nullptr, scan, nullptr);
    return hipGetLastError();
}

hipError_t launch_encode_small(hipStream_t s, const uint8_t* payload, const wsg_send_desc* desc, uint32_t n,
                               uint64_t* wire_off, const uint64_t* scan, uint8_t* wire, uint64_t wire_cap,
                               unsigned long long* err)
{
    // frames per block: as many as fit SMALL_RANGE wire bytes at the average
    // frame size (wire_cap / n), so that larger frames still fill the grid
    const uint64_t avg = wire_cap / n + 1;
    uint32_t fpb = SMALL_F;
    while (fpb > 1 && uint64_t(fpb) * avg > SMALL_RANGE)
        fpb >>= 1;
    const uint32_t nb = uint32_t((n + SCAN_ITEMS - 1) / SCAN_ITEMS);
    k_encode_small<<<(n + fpb - 1) / fpb, BLOCK, 0, s>>>(payload, desc, n, fpb, wire_off, scan, nb, wire, wire_cap,
                                                         err);
    return hipGetLastError();
}

} // namespace wsg
